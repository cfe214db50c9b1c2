#!/usr/bin/env python3
"""Rate of the dense stereo stage (aria_dense_compute_batch_device: census + four-path SGM over 64 disparities + winner,
uniqueness, left-right check, sub-pixel and depth): rectified pairs resident in HBM at 640x480 and at 752x480, timed with HIP
events on the handle's stream. Two batches per shape: one that fits the pairs the default scratch_bytes keeps in flight
(one group) and one of three and a half times as many (four groups). The inputs are 16 distinct synthetic pairs
(stereo_ref.stereo_pair: row disparities 7, 19.5 and 42.25 px) tiled over the batch on the device -- every pair has its own
images and outputs in memory. Prints microseconds per pair and appends one JSON line per shape and batch to --out.

Usage: dense_rate.py [--shapes 640x480,752x480] [--reps 20] [--warmup 3] [--out profiles/dense_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 16
HBM_PEAK = 8.0e12


def measure(A, torch, W, H, B, reps, warmup):
    from aria_slam_amd import dense
    from aria_slam_amd import stereo_ref as R
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    pairs = [R.stereo_pair(100 + s, W, H) for s in range(DISTINCT)]
    h = A.HipDenseStereo(max_size=(W, H), stream=stream.cuda_stream)
    G = h.pairs_in_flight
    if B is None:
        B = G
    reps_of = (B + DISTINCT - 1) // DISTINCT
    with torch.cuda.stream(stream):
        left = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev).repeat((reps_of, 1, 1))[:B].contiguous()
        right = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev).repeat((reps_of, 1, 1))[:B].contiguous()
        disp = torch.zeros((B, H, W), dtype=torch.int16, device=dev)
        depth = torch.zeros((B, H, W), dtype=torch.float32, device=dev)
    stream.synchronize()

    def run():
        h.compute_batch_device(left, right, W, H, B, disp, depth)

    for _ in range(warmup):
        run()
    h.check()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(stream)
        run()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    h.check()
    ms = float(np.median(times))
    valid = float((disp[:DISTINCT, :, 64:] > 0).float().mean().item())
    alg = dense.algorithmic_bytes(W, H)
    res = dict(width=W, height=H, pairs=B, pairs_in_flight=G, groups=(B + G - 1) // G, ms_median=ms, ms_min=float(np.min(times)),
               ms_max=float(np.max(times)), us_per_pair=ms * 1e3 / B, algorithmic_bytes_per_pair=alg,
               algorithmic_share_of_hbm_peak=alg * B / (ms * 1e-3) / HBM_PEAK,
               scratch_bytes_per_pair=dense.scratch_bytes_per_pair(W, H), valid_share_x_ge_64=valid)
    print("%dx%d, %d pairs in %d group(s) of <= %d: %.3f ms (median of %d, min %.3f max %.3f) = %.1f us/pair, valid share %.4f"
          % (W, H, B, res["groups"], G, ms, reps, res["ms_min"], res["ms_max"], res["us_per_pair"], valid))
    print(json.dumps(res))
    h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="640x480,752x480")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_rate.json"))
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    assert torch.cuda.is_available(), "dense_rate.py measures on the GPU; there is no CPU fallback"
    results = []
    for shape in a.shapes.split(","):
        W, H = (int(v) for v in shape.split("x"))
        one = measure(A, torch, W, H, None, a.reps, a.warmup)
        results.append(one)
        results.append(measure(A, torch, W, H, one["pairs_in_flight"] * 7 // 2, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
