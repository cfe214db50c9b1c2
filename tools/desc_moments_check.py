"""The batch k_describe's moment phase against the oracle, byte for byte: keypoint records (angle included) and descriptors of
every keypoint. The cases aim at what the matrix-core phase (describe16<0>, v_mfma_i32_16x16x64_i8 on byte-exact 16-byte
window loads) can get wrong and the 16-keypoint layout tests (tools/describe16_check.py) do not look for:

  pair      : 2 frames of 320x240, 500 features
  unaligned : 2 frames of 321x241 whose device pointer is 1 byte past an allocation: the rows of level 0 start at every
              alignment, so do the window loads
  rects     : random 0 / 255 rectangles: saturated moments of both signs (the int8 products at their extremes)
  edges     : corners planted at x = 31, x = w - 32, y = 31, y = h - 32 with random stripes under the outermost window bytes:
              the first and last byte of a window row, the first and last row

Prints one "OK <case>" line per case; exits non-zero on the first difference. Run in-process by tests/test_gpu_desc_mfma.py
for the product library and, through ARIA_ORB_HIP_LIBRARY, as a program against the -DARIA_DESC_MOMENTS_LDS=1 build
(tools/build_ab.sh), which keeps the LDS moment rounds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import aria_slam_amd as A  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

NF = 500


def run_batch(imgs, nf, lead=0):
    """extract_batch_device on `imgs`, the device image `lead` bytes past its allocation; (counts, kps, desc, kernel name)."""
    dev = torch.device("cuda", 0)
    B, h, w = imgs.shape
    e = A.OrbHipExtractor(max_features=nf, max_width=w, max_height=h, max_batch=B)
    try:
        cap = e.kp_capacity()
        kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device=dev)
        desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
        cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
        flat = torch.zeros((lead + B * h * w,), dtype=torch.uint8, device=dev)
        d_img = flat[lead:]
        d_img.copy_(torch.from_numpy(np.ascontiguousarray(imgs).reshape(-1)))
        assert d_img.data_ptr() == flat.data_ptr() + lead
        torch.cuda.synchronize()
        e.extract_batch_device(d_img, B, w, h, kps, desc, cnt, cap)
        e.check()
        return cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy(), e.fast_blur_kernel()
    finally:
        e.close()


def check(imgs, nf=NF, lead=0):
    """Every keypoint of every frame, none left out; returns the oracle's records per frame."""
    p = O.default_params(nf)
    want = [O.orb_extract(im, p) for im in imgs]
    cnt, kps, desc, kernel = run_batch(imgs, nf, lead)
    assert kernel == "k_fast_blur_stream", kernel                  # the Q4 batch path (the form under test)
    for f, (ok, od) in enumerate(want):
        n = len(ok)
        assert n > 0 and cnt[f] == n, (f, cnt[f], n)
        got = np.frombuffer(kps[f, :n].tobytes(), dtype=ok.dtype)
        if got.tobytes() != ok.tobytes():
            bad = [i for i in range(n) if got[i].tobytes() != ok[i].tobytes()]
            raise AssertionError("frame %d: %d of %d keypoint records differ, first %d: got %s, oracle %s"
                                 % (f, len(bad), n, bad[0], got[bad[0]], ok[bad[0]]))
        assert np.array_equal(desc[f, :n], od), "frame %d: descriptors differ" % f
    return [w[0] for w in want]


def case_pair():
    a, b = A.synth_frame_pair(71, 320, 240)
    check(np.stack([a, b]))
    print("OK pair")


def case_unaligned():
    a, b = A.synth_frame_pair(72, 321, 241)
    check(np.stack([a, b]), lead=1)
    print("OK unaligned")


def _rects(seed, w, h):
    r = np.random.RandomState(seed)
    img = np.zeros((h, w), np.uint8)
    for _ in range(220):
        x0, y0 = int(r.randint(0, w - 4)), int(r.randint(0, h - 4))
        rw, rh = int(r.randint(4, 48)), int(r.randint(4, 48))
        img[y0:y0 + rh, x0:x0 + rw] = 255 * int(r.randint(0, 2))
    return img


def case_rects():
    w, h = 320, 240
    imgs = np.stack([_rects(5, w, h), _rects(6, w, h)])
    kps = check(imgs)
    # the case is about saturated windows of both signs: both half-planes of angles occur
    ang = np.concatenate([k["angle"] for k in kps])
    assert (ang < 90).any() and ((ang > 90) & (ang < 270)).any() and (ang > 270).any(), "the rectangles gave one-sided moments"
    print("OK rects")


def _edges(seed, w, h):
    r = np.random.RandomState(seed)
    img = r.randint(40, 57, size=(h, w)).astype(np.uint8)           # flat enough that the noise alone makes no FAST corner
    # random stripes under the outermost bytes of the windows of keypoints on the border of the valid region
    img[:, 16] = r.randint(0, 256, size=h)
    img[:, w - 17] = r.randint(0, 256, size=h)
    img[16, :] = r.randint(0, 256, size=w)
    img[h - 17, :] = r.randint(0, 256, size=w)
    # isolated bright pixels are FAST corners where they stand; distinct values keep their scores apart
    pts = [(31, y) for y in range(31, h - 31, 14)] + [(w - 32, y) for y in range(38, h - 31, 14)]
    pts += [(x, 31) for x in range(45, w - 32, 14)] + [(x, h - 32) for x in range(52, w - 32, 14)]
    pts += [(w - 32, h - 32), (w - 32, 31), (31, h - 32)]
    for i, (x, y) in enumerate(pts):
        img[y, x] = 150 + (i * 37) % 106
    return img


def case_edges():
    w, h = 320, 240
    imgs = np.stack([_edges(1, w, h), _edges(2, w, h)])
    kps = check(imgs)
    for k in kps:                                                    # the planted corners are among the results, on level 0
        k0 = k[k["octave"] == 0]
        for name, hit in (("x = 31", k0["x"] == 31), ("x = w - 32", k0["x"] == w - 32), ("y = 31", k0["y"] == 31),
                          ("y = h - 32", k0["y"] == h - 32)):
            assert hit.sum() >= 4, "no planted corners at %s in the result" % name
    print("OK edges")


CASES = ["pair", "unaligned", "rects", "edges"]

if __name__ == "__main__":
    A.load_library()
    O.build()
    O.lib()
    for c in sys.argv[1:] or CASES:
        globals()["case_" + c]()
