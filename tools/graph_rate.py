#!/usr/bin/env python3
"""Rate of the batched pose-graph stage (aria_graph_optimize_batch_device): a batch of 256 graphs x 512 vertices x 8 loop
edges and one graph of 3000 vertices x 5 loop edges (circle scenes of aria_slam_amd.graph_ref, noisy odometry with a yaw
bias), 10 LM iterations, timed with HIP events on the optimizer's stream (median of 20; the poses are restored on the same
stream before every call, outside the timed interval). Prints ms per call, PCG iterations and microseconds per PCG iteration
per graph, beside graph_ref(solver="direct") on the host for the same graphs (16 processes over 16 of the batch's graphs; the
stand-in for what the reference spends in g2o), and one JSON line per case.

Usage: graph_rate.py [--graphs 256] [--vertices 512] [--loops 8] [--big 3000] [--big-loops 5] [--iterations 10] [--reps 20]
                     [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _scene(args):
    from aria_slam_amd import graph_ref as G
    seed, n, loops, laps = args
    _truth, init, odo, lp = G.circle_scene(seed, n=n, laps=laps, n_loops=loops)
    return init, odo + lp


def _host(args):
    from aria_slam_amd import graph_ref as G
    init, edges, its = args
    t = time.perf_counter()
    _P, r = G.optimize(init, edges, 0, its, "direct")
    return time.perf_counter() - t, r["chi2_final"]


def measure(A, torch, graphs, iterations, reps, warmup, max_graphs):
    from aria_slam_amd.posegraph import pack_edges, pack_poses
    from aria_slam_amd._lib import GRAPH_RESULT_DTYPE
    dev = torch.device("cuda", 0)
    B = len(graphs)
    rows = [pack_poses(g[0]) for g in graphs]
    recs = [pack_edges(g[1]) for g in graphs]
    voff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    eoff = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
    pristine, dv, de, do = d(np.concatenate(rows)), d(voff), d(np.concatenate(recs)), d(eoff)
    df = torch.zeros(B, dtype=torch.int32, device=dev)
    dp = pristine.clone()
    dres = torch.zeros(B * GRAPH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    opt = A.HipPoseGraphOptimizer(max_vertices=max(len(r) for r in rows), max_edges=max(len(r) for r in recs),
                                  max_graphs=max_graphs, stream=stream.cuda_stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):
        with torch.cuda.stream(stream):
            dp.copy_(pristine)
        t0.record(stream)
        opt.optimize_batch_device(dp, dv, de, do, df, B, iterations, dres)
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    opt.check()
    res = np.frombuffer(dres.cpu().numpy().tobytes(), GRAPH_RESULT_DTYPE)
    opt.close()
    return float(np.median(times)), float(np.min(times)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--vertices", type=int, default=512)
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--big", type=int, default=3000)
    ap.add_argument("--big-loops", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import multiprocessing as mp
    import torch
    import aria_slam_amd as A

    with mp.get_context("spawn").Pool(16) as pool:      # before the GPU is opened in this process; the workers never open it
        distinct = pool.map(_scene, [(100 + s, a.vertices, a.loops, 1.5) for s in range(16)])
        big = _scene((200, a.big, a.big_loops, 2.0))
        host = {}
        if not a.no_host:
            t = time.perf_counter()
            per = pool.map(_host, [(g[0], g[1], a.iterations) for g in distinct])
            host["batch_wall_s_16_graphs_16_processes"] = time.perf_counter() - t
            host["batch_s_per_graph_one_process"] = float(np.mean([p[0] for p in per]))
            host["big_s"] = _host((big[0], big[1], a.iterations))[0]

    cases = [("batch", [distinct[g % 16] for g in range(a.graphs)], a.graphs), ("big", [big], 1)]
    for name, graphs, slots in cases:
        ms, ms_min, res = measure(A, torch, graphs, a.iterations, a.reps, a.warmup, slots)
        B = len(graphs)
        pcg = float(res["pcg_iterations"].mean())
        out = dict(case=name, graphs=B, vertices=len(graphs[0][0]), edges=len(graphs[0][1]), iterations=a.iterations,
                   ms_median=ms, ms_min=ms_min, ms_per_graph=ms / B, pcg_iterations_per_graph=pcg,
                   us_per_pcg_iteration=ms * 1e3 / max(pcg, 1), us_per_pcg_iteration_per_graph=ms * 1e3 / max(pcg, 1) / B,
                   valid=int(res["valid"].sum()), iterations_done=float(res["iterations_done"].mean()),
                   trials=float(res["trials"].mean()), chi2_initial=float(res["chi2_initial"].mean()),
                   chi2_final=float(res["chi2_final"].mean()))
        if host:
            if name == "batch":
                out["host_direct_s_per_graph_16_processes"] = host["batch_wall_s_16_graphs_16_processes"] / 16
                out["host_direct_s_per_graph_one_process"] = host["batch_s_per_graph_one_process"]
            else:
                out["host_direct_s_per_graph_one_process"] = host["big_s"]
        print("%s: %d graph%s x %d vertices x %d edges, %d iterations: %.3f ms per call (median of %d), %.1f PCG iterations per "
              "graph, %.2f us per PCG iteration, %.3f us per PCG iteration per graph, %.3f ms per graph%s" %
              (name, B, "" if B == 1 else "s", out["vertices"], out["edges"], a.iterations, ms, a.reps, pcg,
               out["us_per_pcg_iteration"], out["us_per_pcg_iteration_per_graph"], out["ms_per_graph"],
               "; host direct solve %.1f ms per graph" % (1e3 * out.get("host_direct_s_per_graph_16_processes",
                                                                          out.get("host_direct_s_per_graph_one_process", 0)))
               if host else ""))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
