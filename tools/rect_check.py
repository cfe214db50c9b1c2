#!/usr/bin/env python3
"""The remap cases of tests/rectify_cases.py (EDGE_CASES: both sides of every term of k_rect_remap's choice between its read
forms, three frame groups, the limits of the map word, and zoom20_big, whose 64 x 16 tiles do and do not fit the LDS of
k_rect_remap_lds) through whatever library ARIA_ORB_HIP_LIBRARY names, each held bitwise to the restatement
(aria_slam_amd/rectify_ref.py). With the variants build the switches ARIA_RECT_READ (taps, lds) and ARIA_RECT_GROUP, read when
a handle is created, select the kernel and the frame group; the product library knows no switch. Prints one line per case,
"<case>: 0 of N pixels differ", and exits non-zero on a difference or a written padding byte.
tests/test_gpu_rectify_variants.py runs it once per setting."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import aria_slam_amd as A
    import rectify_cases as RC
    assert torch.cuda.is_available(), "rect_check.py runs on the GPU; there is no CPU fallback"
    print("library %s, ARIA_RECT_READ=%s ARIA_RECT_GROUP=%s" % (os.path.basename(A.library_path()), os.environ.get("ARIA_RECT_READ", ""),
                                                               os.environ.get("ARIA_RECT_GROUP", "")))
    switched = [k for k in ("ARIA_RECT_READ", "ARIA_RECT_GROUP") if os.environ.get(k)]
    assert not switched or A.library_path().endswith("libaria_orb_hip_variants.so"), \
        "%s is read by the variants build only: the product library would run the shipped kernel under its name" % switched[0]
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    wrong = 0
    for name, case in RC.EDGE_CASES.items():
        r = A.HipRectifier(cameras=case.cam, new_K=case.new_K, src_size=case.src, dst_size=case.dst, fill=case.fill,
                           stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_src = torch.from_numpy(case.src_buffer().reshape(-1)).to("cuda:0")
            d_dst = torch.full((case.n_frames * case.dst_stride,), 0x5A, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
        r.remap_batch_device(d_src, case.n_frames, d_dst, 0, case.src_stride, case.src_pitch, case.dst_stride, case.dst_pitch)
        r.check()
        img, pad_kept = case.images(d_dst.cpu().numpy())
        r.close()
        differ = int((img != case.want).sum())
        print("%s: %d of %d pixels differ%s" % (name, differ, case.want.size, "" if pad_kept else ", padding was written"))
        wrong += differ + (0 if pad_kept else 1)
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
