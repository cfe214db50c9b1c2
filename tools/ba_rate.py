#!/usr/bin/env python3
"""Rate of the batched bundle-adjustment stage (aria_ba_optimize_batch_device) at three shapes -- 256 windows x 16 poses x
2000 points x about 8 observations per point, one window of that shape, and 4096 windows x 8 poses x 300 points -- timed
with HIP events on the adjuster's stream (median of 20; poses and points are restored on the same stream before every call,
outside the timed interval), beside ba_ref.optimize on the host for one window of each shape. Also the track builder
(aria_ba_window_from_chain_device) over 64 windows of a generated four-pair chain of 2000 keypoints per frame. Prints one
line and one JSON line per case.

Usage: ba_rate.py [--iterations 10] [--reps 20] [--warmup 2] [--no-host] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(A, torch, windows, B, iterations, reps, warmup):
    from aria_slam_amd._lib import BA_OBS_DTYPE, BA_RESULT_DTYPE
    from aria_slam_amd.bundle import _arrays
    dev = torch.device("cuda", 0)
    arr = [_arrays(w) for w in windows]
    Pc, Nc, Oc = (max(len(a[k]) for a in arr) for k in (0, 2, 4))
    poses, pf = np.zeros((B, Pc, 12)), np.zeros((B, Pc), np.uint8)
    pts, xf = np.zeros((B, Nc, 3)), np.zeros((B, Nc), np.uint8)
    obs, counts = np.zeros((B, Oc), BA_OBS_DTYPE), np.zeros((3, B), np.int32)
    for b in range(B):
        a = arr[b % len(arr)]
        poses[b, :len(a[0])], pf[b, :len(a[1])], pts[b, :len(a[2])], xf[b, :len(a[3])], obs[b, :len(a[4])] = a
        counts[:, b] = (len(a[0]), len(a[2]), len(a[4]))
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    p0, x0, dpf, dxf, do, dn = d(poses), d(pts), d(pf), d(xf), d(obs), d(counts)
    dp, dx = p0.clone(), x0.clone()
    dres = torch.zeros(B * BA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ba = A.HipBundleAdjuster(max_windows=B, stream=stream.cuda_stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):
        with torch.cuda.stream(stream):
            dp.copy_(p0)
            dx.copy_(x0)
        t0.record(stream)
        ba.optimize_batch_device(dp, dpf, dx, dxf, do, dn.data_ptr(), dn.data_ptr() + 4 * B, dn.data_ptr() + 8 * B, B, Pc, Nc, Oc,
                                 iterations, dres)
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    ba.check()
    res = np.frombuffer(dres.cpu().numpy().tobytes(), BA_RESULT_DTYPE)
    ba.close()
    return float(np.median(times)), float(np.min(times)), res, int(counts[2].mean())


def measure_builder(A, torch, reps, warmup, n=2000, windows=64):
    import ba_cases as BC
    kps, matches, nm, ext, _win, _truth = BC.generated_chain(seed=5, n=n)
    frames, P, cap = kps.shape[0], kps.shape[0] - 1, matches.shape[1]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    mp = A.HipMapper(stream=stream.cuda_stream)
    ba = A.HipBundleAdjuster(stream=stream.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    pcap, ocap = P * n, P * n * frames
    with torch.cuda.stream(stream):
        d_k1, d_k2, d_m, d_nm = up(kps[:-1]), up(kps[1:]), up(matches), up(nm)
        d_n, d_ext = up(np.full(P, n, np.int32)), up(ext)
        d_first, d_np = up(np.full(windows, 0, np.int32)), up(np.full(windows, P, np.int32))
        d_X = torch.zeros(windows * pcap * 3, dtype=torch.float64, device=dev)
        d_obs = torch.zeros(windows * ocap * 16, dtype=torch.uint8, device=dev)
        d_src = torch.zeros(windows * pcap, dtype=torch.int32, device=dev)
        d_cnt = torch.zeros((2, windows), dtype=torch.int32, device=dev)
    stream.synchronize()
    mp.triangulate_batch_device(d_k1, d_n, d_k2, d_n, n, d_m, d_nm, P, cap, d_extrinsics=d_ext, query_is_first=True, pair_base=0)
    mp.check()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):
        t0.record(stream)
        ba.window_from_chain_device(mp, d_first, d_np, windows, 0, P, d_k1, d_n, d_k2, d_n, n, d_m, d_nm, cap, pcap, ocap, d_X, d_obs,
                                    d_src, d_cnt[0], d_cnt[1])
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    ba.check()
    cnt = d_cnt.cpu().numpy()
    size = mp.size()
    ba.close()
    mp.close()
    return dict(case="track_builder", windows=windows, pairs=P, keypoints=n, map_points=int(size), points=int(cnt[0, 0]),
                observations=int(cnt[1, 0]), ms_median=float(np.median(times)), ms_min=float(np.min(times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--small", action="store_true", help="a tenth of every batch: a quick look")
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import ba_ref as B

    big = [B.random_window(300 + s, poses=16, points=2000, visibility=(4, 12), pose_noise=0.05, point_noise=0.2)[0] for s in range(8)]
    small = [B.random_window(400 + s, poses=8, points=300, visibility=(2, 8), pose_noise=0.05, point_noise=0.2)[0] for s in range(16)]
    scale = 10 if a.small else 1
    cases = [("batch", big, 256 // scale), ("single", big[:1], 1), ("many_small", small, 4096 // scale)]
    for name, wins, n in cases:
        ms, ms_min, res, nobs = measure(A, torch, wins, n, a.iterations, a.reps, a.warmup)
        out = dict(case=name, windows=n, poses=len(wins[0]["poses"]), points=len(wins[0]["points"]), observations=nobs,
                   iterations=a.iterations, ms_median=ms, ms_min=ms_min, ms_per_window=ms / n, valid=int(res["valid"].sum()),
                   iterations_done=float(res["iterations_done"].mean()), trials=float(res["trials"].mean()),
                   us_per_trial_per_window=ms * 1e3 / max(float(res["trials"].mean()), 1) / n,
                   chi2_initial=float(res["chi2_initial"].mean()), chi2_final=float(res["chi2_final"].mean()),
                   rms_px=float(res["rms_px"].mean()))
        if not a.no_host:
            t = time.perf_counter()
            _p, _x, r = B.optimize(wins[0], a.iterations)
            out["host_restatement_s_per_window"] = time.perf_counter() - t
            out["host_chi2_final"] = r["chi2_final"]
        print("%s: %d window%s x %d poses x %d points x %d observations, %d iterations: %.3f ms per call (median of %d), %.3f ms "
              "per window, %.1f trials%s" % (name, n, "" if n == 1 else "s", out["poses"], out["points"], nobs, a.iterations, ms,
                                            a.reps, ms / n, out["trials"],
                                            "; restatement %.2f s per window" % out["host_restatement_s_per_window"]
                                            if not a.no_host else ""))
        print(json.dumps(out))
    out = measure_builder(A, torch, a.reps, a.warmup)
    print("track builder: %d windows x %d pairs over a map of %d points: %.3f ms per call (median of %d)" %
          (out["windows"], out["pairs"], out["map_points"], out["ms_median"], a.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
