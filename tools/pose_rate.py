#!/usr/bin/env python3
"""Rate of the batched two-view pose stage (aria_pose_estimate_batch_device): 4096 pairs x 600 matches (40 % outliers) at 1024
hypotheses by default, timed with HIP events on the estimator's stream. Prints microseconds per pair and hypothesis
evaluations (Sampson tests) per second, and one JSON line.

Usage: pose_rate.py [--pairs 4096] [--matches 600] [--outliers 0.4] [--hypotheses 1024] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--matches", type=int, default=600)
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import pose_ref as P

    dev = torch.device("cuda", 0)
    n, B = a.matches, a.pairs
    # 64 distinct synthetic scenes (forward / sideways / rotating motions, 2-20 m, 0.5 px noise), tiled over the batch
    scenes = []
    for s in range(64):
        ang = 15.0 * (s % 4) / 3.0
        R = P.rot([0.1 * (s % 3), 1.0, 0.2], ang)
        t = np.array([np.cos(s), 0.2 * np.sin(3 * s), 1.0 + 0.5 * np.sin(s)])
        kq, kt, m, _ = P.synth_two_view(1000 + s, n, R, t / np.linalg.norm(t), a.outliers)
        scenes.append((kq.view(np.uint8).reshape(n, 24), kt.view(np.uint8).reshape(n, 24), m.view(np.uint8).reshape(n, 12)))
    kq = np.stack([scenes[p % 64][0] for p in range(B)])
    kt = np.stack([scenes[p % 64][1] for p in range(B)])
    mm = np.stack([scenes[p % 64][2] for p in range(B)])
    cnt = np.full(B, n, np.int32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dkq, dkt, dmm, dn = d(kq), d(kt), d(mm), d(cnt)
    out = torch.zeros(B * 192, dtype=torch.uint8, device=dev)
    mask = torch.zeros(B * n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    est = A.HipPoseEstimator(hypotheses=a.hypotheses, stream=stream.cuda_stream)

    def run():
        est.estimate_batch_device(dkq, dn, dkt, dn, n, dmm, dn, B, n, out, mask)

    for _ in range(a.warmup):
        run()
    est.check()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.reps):
        t0.record(stream)
        run()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    est.check()
    rec = np.frombuffer(out.cpu().numpy().tobytes(), A._lib.POSE_RESULT_DTYPE)
    ms = float(np.median(times))
    evals = float(B) * a.hypotheses * n
    res = dict(pairs=B, matches=n, outliers=a.outliers, hypotheses=a.hypotheses, ms_median=ms, ms_min=float(np.min(times)), ms_max=float(np.max(times)),
               us_per_pair=ms * 1e3 / B, sampson_evals_per_s=evals / (ms * 1e-3), valid=int(rec["valid"].sum()),
               mean_inliers=float(rec["n_inliers"].mean()), mean_pose_inliers=float(rec["n_pose_inliers"].mean()))
    print("%d pairs x %d matches, %d hypotheses: %.3f ms (median of %d), %.3f us/pair, %.3g hypothesis evaluations/s"
          % (B, n, a.hypotheses, ms, a.reps, res["us_per_pair"], res["sampson_evals_per_s"]))
    print(json.dumps(res))
    est.close()


if __name__ == "__main__":
    main()
