#!/usr/bin/env python3
"""Rate of the batched absolute pose stage (aria_pnp_estimate_batch_device): 4096 pairs x 600 correspondences (40 % outliers)
at 1024 hypotheses by default -- the shape of tools/pose_rate.py -- timed with HIP events on the estimator's stream, median of
20. Also the association call (aria_pnp_associate_batch_device) of the same 4096 pairs against a map that the batch
triangulation of 4096 two-view scenes x 600 matches leaves in HBM (about 2 M points). Prints one JSON line.

--solver dlt|p3p chooses the minimal solver (default dlt). --solver both times the two solvers on one handle in one process,
alternating launch by launch (the solver is a launch parameter), and prints one JSON line per solver, each with the valid
hypotheses per pair of the 64 distinct scenes (aria_pnp_debug_hypotheses) and, for P3P, the smallest H of --sweep at which its
mean inlier count reaches the DLT's at --hypotheses. --planar puts every scene on one plane (the DLT then finds no pose).

Usage: pnp_rate.py [--pairs 4096] [--corr 600] [--outliers 0.4] [--hypotheses 1024] [--reps 20] [--solver dlt|p3p|both]
                   [--planar] [--sweep 64,128,256,512,1024] [--no-assoc]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(torch, stream, fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--corr", type=int, default=600)
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--solver", choices=("dlt", "p3p", "both"), default="dlt")
    ap.add_argument("--planar", action="store_true")
    ap.add_argument("--sweep", default="64,128,256,512,1024")
    ap.add_argument("--no-assoc", action="store_true")
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import pnp_ref as N
    from aria_slam_amd import pose_ref as P

    dev = torch.device("cuda", 0)
    n, B = a.corr, a.pairs
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    # 64 distinct synthetic scenes (2-20 units, 0.5 px noise), tiled over the batch
    poses = []
    for s in range(64):
        R = P.rot([0.1 * (s % 3), 1.0, 0.2], 15.0 * (s % 4) / 3.0)
        poses.append((R, np.array([np.cos(s), 0.2 * np.sin(3 * s), 1.0 + 0.5 * np.sin(s)])))
    scenes = [N.synth_pnp(1000 + s, n, R, t, a.outliers, planar=a.planar)[0].view(np.uint8).reshape(n, 32)
              for s, (R, t) in enumerate(poses)]
    dcorr = d(np.stack([scenes[p % 64] for p in range(B)]))
    dn = d(np.full(B, n, np.int32))
    out = torch.zeros(B * 128, dtype=torch.uint8, device=dev)
    mask = torch.zeros(B * n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    est = A.HipPnPEstimator(hypotheses=a.hypotheses, stream=stream.cuda_stream)
    solvers = ["dlt", "p3p"] if a.solver == "both" else [a.solver]

    def run():
        est.estimate_batch_device(dcorr, dn, B, n, out, mask)

    def summary(hyp):
        rec = np.frombuffer(out.cpu().numpy().tobytes(), A._lib.PNP_RESULT_DTYPE)
        return dict(pairs=B, corr=n, outliers=a.outliers, hypotheses=hyp, planar=bool(a.planar), valid=int(rec["valid"].sum()),
                    mean_inliers=float(rec["n_inliers"].mean()), mean_iterations=float(rec["iterations"].mean()))

    times = {k: [] for k in solvers}
    results = {}
    for k in solvers:
        est.solver = k
        for _ in range(a.warmup):
            run()
        est.check()
    for _ in range(a.reps):                                      # alternating, launch by launch
        for k in solvers:
            est.solver = k
            times[k] += _time(torch, stream, run, 1)
    est.check()
    for k in solvers:
        est.solver = k
        run()
        est.check()
        ms = float(np.median(times[k]))
        r = summary(a.hypotheses)
        r.update(solver=k, ms_median=ms, ms_min=float(np.min(times[k])), ms_max=float(np.max(times[k])), us_per_pair=ms * 1e3 / B,
                 evals_per_s=float(B) * a.hypotheses * n / (ms * 1e-3))
        if a.solver == "both":
            nv = [int((est.debug_hypotheses(np.frombuffer(sc.tobytes(), A._lib.PNP_CORR_DTYPE))[3] >= 0).sum()) for sc in scenes]
            r["valid_hypotheses_per_pair"] = float(np.mean(nv))
        results[k] = r
        print("%s: %d pairs x %d correspondences, %d hypotheses: %.3f ms (median of %d), %.3f us/pair, %.3g reprojection tests/s"
              % (k, B, n, a.hypotheses, ms, a.reps, r["us_per_pair"], r["evals_per_s"]))
    if a.solver == "both":
        target = results["dlt"]["mean_inliers"]
        sweep = []
        for hyp in sorted(int(v) for v in a.sweep.split(",")):
            e2 = A.HipPnPEstimator(hypotheses=hyp, stream=stream.cuda_stream, solver="p3p")
            e2.estimate_batch_device(dcorr, dn, B, n, out, mask)
            e2.check()
            t2 = _time(torch, stream, lambda: e2.estimate_batch_device(dcorr, dn, B, n, out, mask), 5)
            e2.check()
            sm = summary(hyp)
            sweep.append(dict(hypotheses=hyp, mean_inliers=sm["mean_inliers"], valid=sm["valid"], ms_median=float(np.median(t2))))
            e2.close()
        reach = [w["hypotheses"] for w in sweep if w["mean_inliers"] >= target]
        results["p3p"].update(sweep=sweep, dlt_mean_inliers=target, smallest_h_reaching_dlt=(reach[0] if reach else None))
    for k in solvers[:-1]:
        print(json.dumps(results[k]))
    res = results[solvers[-1]]
    est.solver = "dlt"
    if a.no_assoc:
        print(json.dumps(res))
        est.close()
        return

    # the association: a map from the batch triangulation of B two-view scenes, then B tracked pairs against it
    two = []
    for s, (R, t) in enumerate(poses):
        kq, kt, m, _ = P.synth_two_view(2000 + s, n, R, t / np.linalg.norm(t), 0.0)
        ext = np.concatenate([np.hstack([np.eye(3), np.zeros((3, 1))]).ravel(), np.hstack([R, (t / np.linalg.norm(t))[:, None]]).ravel()])
        two.append((kq.view(np.uint8).reshape(n, 24), kt.view(np.uint8).reshape(n, 24), m.view(np.uint8).reshape(n, 12), ext))
    dkq, dkt, dmm = (d(np.stack([two[p % 64][k] for p in range(B)])) for k in range(3))
    dext = d(np.stack([two[p % 64][3] for p in range(B)]))
    acorr = torch.zeros(B * n * 32, dtype=torch.uint8, device=dev)
    ancorr = torch.zeros(B, dtype=torch.int32, device=dev)
    aback = torch.zeros(B * n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    mp = A.HipMapper(capacity=B * n, stream=stream.cuda_stream)
    mp.triangulate_batch_device(dkq, dn, dkt, dn, n, dmm, dn, B, n, d_extrinsics=dext)
    mp.check()
    size = mp.size()

    def assoc():
        est.associate_batch_device(mp, 0, 2, dkq, dn, n, dmm, dn, B, n, acorr, ancorr, aback)

    for _ in range(a.warmup):
        assoc()
    est.check()
    atimes = _time(torch, stream, assoc, a.reps)
    est.check()
    res.update(map_points=int(size), assoc_ms_median=float(np.median(atimes)), assoc_ms_min=float(np.min(atimes)),
               assoc_ms_max=float(np.max(atimes)), assoc_corr=int(ancorr.sum().item()))
    print("association of %d pairs x %d matches against a map of %d points: %.3f ms (median of %d), %d correspondences"
          % (B, n, size, res["assoc_ms_median"], a.reps, res["assoc_corr"]))
    print(json.dumps(res))
    mp.close()
    est.close()


if __name__ == "__main__":
    main()
