#!/usr/bin/env python3
"""Rate of trajectory evaluation (aria_eval_batch_device, aria_eval_sample_truth_device), timed with HIP events on the
handle's stream (median of 20 after 3 warm-up calls) for
  wide    4096 trajectories x 512 poses       a sweep: one score per graph / noise setting / track
  deep    64 trajectories x 65 536 poses
  single  1 trajectory x 3 600 poses          one EuRoC-length sequence
each HBM-resident (12-double [R t] pose rows as aria_graph_optimize_batch_device leaves them, and packed xyz) and host-fed
(aria_eval_batch on pageable host arrays, wall clock: staging copies included), and for the sampler: 36 000 ground-truth rows,
3 600 and 1 000 000 queries.

Bytes. The three passes read a pose's position and its truth's: 3 x (24 + 24) B useful. What moves is whole lines: a pose row
is 96 B and a truth record 136 B, so [R t] rows touch 3 x (96 + 136) B per pose, packed xyz 3 x (24 + 136) B. Both rates are
printed. The status quo this replaces is copying the poses to the host and scoring them there with aria_slam_amd.eval_ref:
the D2H copy is timed, eval_ref is timed on a few trajectories and scaled (a Python loop: minutes for the wide shape).
One JSON line per case; --out FILE also writes them to a file.

Usage: eval_rate.py [--reps 20] [--warmup 3] [--out profiles/eval_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, stream, reps, warmup, call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):
        t0.record(stream)
        call()
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(np.min(times))


def run_case(A, torch, name, B, n, reps, warmup, ref_us_per_pose):
    from aria_slam_amd import _lib
    from aria_slam_amd import evaluate as EV
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    NP = B * n
    g = np.cumsum(rng.normal(size=(n, 3)) * 0.05, axis=0)
    truth_pos = np.tile(g, (B, 1)) + np.repeat(rng.normal(size=(B, 3)), n, axis=0)
    est = truth_pos * 0.5 + 1.0 + 0.01 * rng.normal(size=(NP, 3))
    rows = np.zeros((NP, 12))
    rows[:, [0, 5, 10]] = 1.0
    rows[:, [3, 7, 11]] = est
    truth = EV.truth_from_positions(truth_pos)
    off = (np.arange(B + 1) * n).astype(np.int32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
    d_rows, d_xyz, d_truth, d_off = d(rows), d(est), d(truth), d(off)
    d_res = torch.zeros(B * _lib.EVAL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ev = A.HipTrajectoryEvaluator(stream=stream.cuda_stream)
    out = dict(case=name, trajectories=B, poses_each=n, poses=NP)
    for kind, label, d_est, touched in ((_lib.EVAL_EST_POSE12, "pose12", d_rows, 3 * (96 + 136)), (_lib.EVAL_EST_XYZ, "xyz", d_xyz, 3 * (24 + 136))):
        ms, ms_min = timed(torch, stream, reps, warmup,
                           lambda: ev.evaluate_batch_device(d_est, kind, d_off, NP, B, d_truth, NP, d_res))
        ev.check()
        out["%s_ms_median" % label], out["%s_ms_min" % label] = ms, ms_min
        out["%s_traj_per_s" % label], out["%s_poses_per_s" % label] = B / (ms * 1e-3), NP / (ms * 1e-3)
        out["%s_useful_GBps" % label] = NP * 3 * 48 / (ms * 1e-3) * 1e-9
        out["%s_touched_GBps" % label] = NP * touched / (ms * 1e-3) * 1e-9
        print("%s %s resident: %.3f ms (median of %d, min %.3f) | %.3g trajectories/s %.3g poses/s | %.1f GB/s useful, %.1f GB/s of lines touched"
              % (name, label, ms, reps, ms_min, out["%s_traj_per_s" % label], out["%s_poses_per_s" % label],
                 out["%s_useful_GBps" % label], out["%s_touched_GBps" % label]))
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), _lib.EVAL_RESULT_DTYPE)
    out["valid"], out["aligned"] = int(res["valid"].sum()), int(res["align_valid"].sum())
    # host-fed: aria_eval_batch on host arrays, wall clock, staging copies included
    L = A.load_library()
    hres = np.zeros(B, _lib.EVAL_RESULT_DTYPE)
    times = []
    for k in range(2 + 5):
        t = time.perf_counter()
        rc = L.aria_eval_batch(ev._h, rows.ctypes.data, _lib.EVAL_EST_POSE12, off.ctypes.data, NP, B, truth.ctypes.data, NP, 0, None,
                               _lib.EVAL_ALIGN_SIM3, 10, None, hres.ctypes.data)
        assert rc == 0
        if k >= 2:
            times.append((time.perf_counter() - t) * 1e3)
    out["host_fed_ms_median"] = float(np.median(times))
    out["host_fed_traj_per_s"], out["host_fed_poses_per_s"] = B / (out["host_fed_ms_median"] * 1e-3), NP / (out["host_fed_ms_median"] * 1e-3)
    assert hres.tobytes() == res.tobytes()
    # the status quo: poses back to the host (timed), then eval_ref there (scaled from a sample)
    h_rows = torch.empty(d_rows.shape, dtype=torch.uint8).pin_memory()
    with torch.cuda.stream(stream):
        ms_d2h, _ = timed(torch, stream, 5, 1, lambda: h_rows.copy_(d_rows, non_blocking=True))
    out["d2h_ms_median"] = ms_d2h
    out["status_quo_ms_estimate"] = ms_d2h + ref_us_per_pose * NP * 1e-3
    print("%s host-fed: %.3f ms wall (%.3g trajectories/s) | status quo: D2H %.3f ms + eval_ref %.0f ms (scaled from %.1f us per pose)"
          % (name, out["host_fed_ms_median"], out["host_fed_traj_per_s"], ms_d2h, ref_us_per_pose * NP * 1e-3, ref_us_per_pose))
    ev.close()
    return out


def run_sampler(A, torch, n_queries, reps, warmup):
    from aria_slam_amd import _lib, eval_ref as R
    from aria_slam_amd import evaluate as EV
    dev = torch.device("cuda", 0)
    gt = R.truth_rows(36000, 21)
    q = np.random.default_rng(2).uniform(gt[0, 0] - 1.0, gt[-1, 0] + 1.0, n_queries)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
    d_gt, d_q = d(EV.pack_truth(gt)), d(q)
    d_out = torch.zeros(n_queries * 136, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ev = A.HipTrajectoryEvaluator(stream=stream.cuda_stream)
    ms, ms_min = timed(torch, stream, reps, warmup, lambda: ev.sample_ground_truth_device(d_gt, len(gt), d_q, n_queries, d_out))
    ev.check()
    ev.close()
    out = dict(case="sampler", rows=len(gt), queries=n_queries, ms_median=ms, ms_min=ms_min, queries_per_s=n_queries / (ms * 1e-3),
               scan_GBps=len(gt) * 136 / (ms * 1e-3) * 1e-9)
    print("sampler: %d rows, %d queries: %.3f ms (median of %d, min %.3f) | %.3g queries/s (the scan of the rows included)"
          % (len(gt), n_queries, ms, reps, ms_min, out["queries_per_s"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from aria_slam_amd import eval_ref as R
    e, g, _ = R.make_track("walk", 512, 1)
    t = time.perf_counter()
    for _ in range(4):
        R.evaluate(e, g)
    ref_us = (time.perf_counter() - t) * 1e6 / (4 * 512)
    print("host: eval_ref.evaluate takes %.1f us per pose in fp64 (a Python loop)" % ref_us)
    import torch
    import aria_slam_amd as A
    results = [run_case(A, torch, "wide", 4096, 512, a.reps, a.warmup, ref_us),
               run_case(A, torch, "deep", 64, 65536, a.reps, a.warmup, ref_us),
               run_case(A, torch, "single", 1, 3600, a.reps, a.warmup, ref_us),
               run_sampler(A, torch, 3600, a.reps, a.warmup), run_sampler(A, torch, 1000000, a.reps, a.warmup)]
    for r in results:
        r["eval_ref_us_per_pose"] = ref_us
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in results) + "\n")


if __name__ == "__main__":
    main()
