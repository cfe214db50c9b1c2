#!/usr/bin/env python3
"""Rate of the object-detector stage's two kernels (aria_slam_amd/csrc/detect_stage.hip) at the evaluation loop's shape:
256 EuRoC-sized gray frames (752 x 480) to a 640 x 640 network input, 300 candidates per frame.

Writes profiles/det_rate.json (or --out): milliseconds per batch of k_det_preprocess (fp32 and fp16 output) and of
k_det_postprocess, each as median / min / max over --reps timed repetitions (of --inner back-to-back launches between two events on the
handle's stream, divided by their number) after --warmup untimed launches; and the preprocess kernel's achieved fraction of the 8 TB/s HBM peak, from its
algorithmic bytes (aria_det_algorithmic_bytes: W * H * C read + 3 * in_w * in_h * element written per frame)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def candidates(n_frames, n, seed=7):
    """Integer boxes over a 640 x 640 canvas with sides up to 160 and scores in 64ths: a head with real overlap and ties."""
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, 600, (n_frames, n)), rng.integers(0, 600, (n_frames, n))
    w, h = rng.integers(8, 160, (n_frames, n)), rng.integers(8, 160, (n_frames, n))
    sc = rng.integers(8, 64, (n_frames, n)) / 64.0
    return np.stack([x, y, x + w, y + h, sc, rng.integers(0, 20, (n_frames, n))], 2).astype(np.float32)


def timed(torch, stream, fn, warmup, reps, inner):
    """Each repetition brackets `inner` back-to-back launches with two events and reports their mean: one launch is a fraction
    of a millisecond, too short to time alone."""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps,
            "launches_per_rep": inner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--input", type=int, default=640)
    ap.add_argument("--candidates", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed repetition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_rate.json"))
    a = ap.parse_args()
    import torch

    import aria_slam_amd as A
    B, W, H, S, NC = a.frames, a.width, a.height, a.input, a.candidates
    L = A.load_library()
    imgs = A.synth_sequence(1, B // 2, W, H)
    d_img = torch.from_numpy(imgs).cuda()
    raw = candidates(B, NC)
    d_raw = torch.from_numpy(raw).cuda()
    d_dets = torch.zeros(B * NC * 24, dtype=torch.uint8, device="cuda")
    d_boxes = torch.zeros(B * NC * 16, dtype=torch.uint8, device="cuda")
    d_nd = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_nb = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {"frames": B, "width": W, "height": H, "input": S, "candidates": NC, "channels": 1, "hbm_peak_bytes_per_s": HBM_PEAK,
           "device": torch.cuda.get_device_name(0)}
    for half in (False, True):
        det = A.HipObjectDetector(input_size=(S, S), max_batch=B, half=half, max_candidates=NC)
        st = torch.cuda.ExternalStream(det.stream)
        det.input_tensor()
        torch.cuda.synchronize()
        r = timed(torch, st, lambda: det.preprocess_batch_device(d_img, B, W, H), a.warmup, a.reps, a.inner)
        det.check()
        nbytes = B * L.aria_det_algorithmic_bytes(W, H, 1, S, S, int(half))
        r["algorithmic_bytes"] = int(nbytes)
        for k in ("median", "min", "max"):
            r["hbm_fraction_at_%s" % k] = nbytes / (r[k + "_ms"] * 1e-3) / HBM_PEAK
        r["frames_per_s_at_median"] = B / (r["median_ms"] * 1e-3)
        res["preprocess_f16" if half else "preprocess_f32"] = r
        if not half:
            r = timed(torch, st, lambda: det.postprocess_batch_device(d_raw, B, NC, W, H, d_dets, d_nd, NC, d_boxes, d_nb, NC),
                      a.warmup, a.reps, a.inner)
            assert det.status() == (0, 0, 0)
            r["frames_per_s_at_median"] = B / (r["median_ms"] * 1e-3)
            r["kept_per_frame_mean"] = float(d_nd.cpu().numpy().mean())
            res["postprocess"] = r
        det.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
