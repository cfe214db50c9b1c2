#!/usr/bin/env python3
"""Rate of the batched triangulation stage (aria_map_triangulate_batch_device: triangulation + append into the HBM map):
4096 pairs x 600 matches (20 % outliers) by default, timed with HIP events on the mapper's stream. The map is cleared
before every timed call (aria_map_clear, outside the events). Prints microseconds per pair and points per second, and
one JSON line.

Usage: map_rate.py [--pairs 4096] [--matches 600] [--outliers 0.2] [--reps 20]"""
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
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import map_ref as M

    dev = torch.device("cuda", 0)
    n, B = a.matches, a.pairs
    # 64 distinct synthetic scenes (baselines 0.5-1.5, 5-15 degree rotations, 1-20 units, 0.5 px noise), tiled over the batch
    scenes = []
    for s in range(64):
        R1 = M.rot([0.1 * (s % 3), 1.0, 0.2], 3.0 * (s % 5))
        E1 = M.extrinsics(R1, [0.1 * np.cos(s), 0.2, 0.1])
        R2 = M.rot([0.2, 1.0, 0.1 * (s % 4)], 5.0 + 10.0 * (s % 3) / 2.0) @ R1
        E2 = M.extrinsics(R2, [-0.5 - (s % 3) * 0.5, 0.1 * np.sin(s), 0.2])
        kq, kt, m, _, _ = M.synth_scene(1000 + s, n, E1, E2, a.outliers, depth=(1.0, 20.0))
        scenes.append((kq.view(np.uint8).reshape(n, 24), kt.view(np.uint8).reshape(n, 24), m.view(np.uint8).reshape(n, 12),
                       np.concatenate([E1.reshape(-1), E2.reshape(-1)])))
    kq = np.stack([scenes[p % 64][0] for p in range(B)])
    kt = np.stack([scenes[p % 64][1] for p in range(B)])
    mm = np.stack([scenes[p % 64][2] for p in range(B)])
    ext = np.stack([scenes[p % 64][3] for p in range(B)])
    cnt = np.full(B, n, np.int32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dkq, dkt, dmm, dn, dext = d(kq), d(kt), d(mm), d(cnt), d(ext)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    mp = A.HipMapper(stream=stream.cuda_stream, capacity=B * n)

    def run():
        mp.triangulate_batch_device(dkq, dn, dkt, dn, n, dmm, dn, B, n, d_extrinsics=dext)

    for _ in range(a.warmup):
        mp.clear()
        run()
    mp.check()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.reps):
        mp.clear()
        t0.record(stream)
        run()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    mp.check()
    size = mp.size()
    ms = float(np.median(times))
    res = dict(pairs=B, matches=n, outliers=a.outliers, ms_median=ms, ms_min=float(np.min(times)), us_per_pair=ms * 1e3 / B,
               matches_per_s=float(B) * n / (ms * 1e-3), points=size, points_per_pair=size / B)
    print("%d pairs x %d matches: %.3f ms (median of %d), %.3f us/pair, %d points (%.1f per pair), %.3g matches/s"
          % (B, n, ms, a.reps, res["us_per_pair"], size, res["points_per_pair"], res["matches_per_s"]))
    print(json.dumps(res))
    mp.close()


if __name__ == "__main__":
    main()
