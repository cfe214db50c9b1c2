#!/usr/bin/env python3
"""Rate of the Sim(3) pose-graph stage (aria_sgraph_optimize_batch_device) beside the SE(3) stage (aria_graph_*) at the same
shapes in the same session, after tools/graph_rate.py: a batch of 256 graphs x 512 vertices x 8 loop edges, one graph of 3000
vertices x 5 loop edges and one graph of 16 vertices x 1 loop edge (circle scenes of aria_slam_amd.graph_ref; the Sim(3) stage
gets the same poses as vertices with s = 1 and the same edges with s = 1), 10 LM iterations, timed with HIP events on the
optimizer's stream (median of 20, the two stages alternating; the vertices are restored on the same stream before every call,
outside the timed interval). Then the map correction (aria_sgraph_correct_points_device) on an arena of 2.4 M points against
its algorithmic bytes, 72 read and 24 written per point. Prints one JSON line per case and writes them all to --out.

Usage: sgraph_rate.py [--graphs 256] [--vertices 512] [--loops 8] [--big 3000] [--big-loops 5] [--small 16] [--iterations 10]
                      [--reps 20] [--points 2400000] [--out profiles/sgraph_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_rate as GR   # noqa: E402


class Runner:
    """One stage on one batch of graphs: buffers on the device, a call timed between two events."""

    def __init__(self, A, torch, graphs, max_graphs, sim3):
        from aria_slam_amd import _lib
        from aria_slam_amd.posegraph import pack_edges, pack_poses
        from aria_slam_amd.sgraph_ref import vertices_from_poses
        from aria_slam_amd.simgraph import pack_sim3_edges, pack_vertices
        self.torch, self.B = torch, len(graphs)
        dev = torch.device("cuda", 0)
        if sim3:
            rows = [pack_vertices(vertices_from_poses(g[0])) for g in graphs]
            recs = [pack_sim3_edges([e + (1.0,) for e in g[1]]) for g in graphs]
            self.rdt = _lib.SGRAPH_RESULT_DTYPE
        else:
            rows, recs, self.rdt = [pack_poses(g[0]) for g in graphs], [pack_edges(g[1]) for g in graphs], _lib.GRAPH_RESULT_DTYPE
        voff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        eoff = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)      # noqa: E731
        self.pristine, self.dv, self.de, self.do = d(np.concatenate(rows)), d(voff), d(np.concatenate(recs)), d(eoff)
        self.df = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.dp = self.pristine.clone()
        self.dres = torch.zeros(self.B * self.rdt.itemsize, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        cls = A.HipSim3GraphOptimizer if sim3 else A.HipPoseGraphOptimizer
        self.opt = cls(max_vertices=max(len(r) for r in rows), max_edges=max(len(r) for r in recs), max_graphs=max_graphs,
                       stream=self.stream.cuda_stream)
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(self, iterations):
        with self.torch.cuda.stream(self.stream):
            self.dp.copy_(self.pristine)
        self.t0.record(self.stream)
        self.opt.optimize_batch_device(self.dp, self.dv, self.de, self.do, self.df, self.B, iterations, self.dres)
        self.t1.record(self.stream)
        self.t1.synchronize()
        return self.t0.elapsed_time(self.t1)

    def finish(self):
        self.opt.check()
        res = np.frombuffer(self.dres.cpu().numpy().tobytes(), self.rdt)
        self.opt.close()
        return res


def compare(A, torch, name, graphs, slots, iterations, reps, warmup):
    runs = {"se3": Runner(A, torch, graphs, slots, False), "sim3": Runner(A, torch, graphs, slots, True)}
    times = {k: [] for k in runs}
    for k in range(warmup + reps):
        for stage, r in runs.items():                     # alternating: both stages see the same minute of the machine
            ms = r.call(iterations)
            if k >= warmup:
                times[stage].append(ms)
    out = dict(case=name, graphs=len(graphs), vertices=len(graphs[0][0]), edges=len(graphs[0][1]), iterations=iterations, reps=reps)
    for stage, r in runs.items():
        res = r.finish()
        ms, pcg = float(np.median(times[stage])), float(res["pcg_iterations"].mean())
        out[stage] = dict(ms_median=ms, ms_min=float(np.min(times[stage])), pcg_iterations_per_graph=pcg,
                          us_per_pcg_iteration=ms * 1e3 / max(pcg, 1), valid=int(res["valid"].sum()),
                          iterations_done=float(res["iterations_done"].mean()), trials=float(res["trials"].mean()),
                          chi2_initial=float(res["chi2_initial"].mean()), chi2_final=float(res["chi2_final"].mean()))
    out["sim3_over_se3_ms"] = out["sim3"]["ms_median"] / out["se3"]["ms_median"]
    out["sim3_over_se3_per_pcg_iteration"] = out["sim3"]["us_per_pcg_iteration"] / out["se3"]["us_per_pcg_iteration"]
    print("%s: %d graph%s x %d vertices x %d edges, %d iterations: SE(3) %.3f ms (%.1f PCG iterations, %.2f us each), Sim(3) %.3f ms "
          "(%.1f, %.2f us each): %.2fx per call, %.2fx per PCG iteration" %
          (name, out["graphs"], "" if out["graphs"] == 1 else "s", out["vertices"], out["edges"], iterations, out["se3"]["ms_median"],
           out["se3"]["pcg_iterations_per_graph"], out["se3"]["us_per_pcg_iteration"], out["sim3"]["ms_median"],
           out["sim3"]["pcg_iterations_per_graph"], out["sim3"]["us_per_pcg_iteration"], out["sim3_over_se3_ms"],
           out["sim3_over_se3_per_pcg_iteration"]))
    print(json.dumps(out))
    return out


def correction(A, torch, n_points, reps, warmup):
    from aria_slam_amd import _lib
    from aria_slam_amd import graph_ref as G
    from aria_slam_amd import sgraph_ref as S
    from aria_slam_amd.simgraph import pack_vertices
    rng = np.random.default_rng(0)
    nv = 1024
    old = np.array([S.vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(0.5, 2)) for _ in range(nv)])
    new = np.array([S.vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(0.5, 2)) for _ in range(nv)])
    pts = np.zeros(n_points, _lib.MAP_POINT_DTYPE)
    pts["X"] = rng.normal(size=(n_points, 3)) * 5
    pts["pair"] = np.arange(n_points) // max(n_points // nv, 1) % nv      # consecutive points share a pair, as a map's do
    dev = torch.device("cuda", 0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)      # noqa: E731
    dp, dt, do, dn = d(pts), d(np.arange(nv, dtype=np.int32)), d(pack_vertices(old)), d(pack_vertices(new))
    dstats = torch.zeros(16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    opt = A.HipSim3GraphOptimizer(max_vertices=16, max_edges=16, stream=stream.cuda_stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):                        # the points keep moving from call to call: the work is the same
        t0.record(stream)
        opt.correct_points_device(dp, n_points, dt, nv, 0, do, dn, nv, dstats)
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    opt.check()
    stats = np.frombuffer(dstats.cpu().numpy().tobytes(), _lib.SGRAPH_STATS_DTYPE)[0]
    opt.close()
    ms = float(np.median(times))
    nbytes = 96 * n_points
    out = dict(case="correct", points=n_points, vertices=nv, reps=reps, ms_median=ms, ms_min=float(np.min(times)),
               algorithmic_bytes=nbytes, gb_per_s=nbytes / (ms * 1e-3) * 1e-9, moved=int(stats["moved"]))
    print("correct: %d points, %.3f ms per call (median of %d), %.1f GB/s of the algorithmic %d bytes (72 read + 24 written per point)"
          % (n_points, ms, reps, out["gb_per_s"], nbytes))
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--vertices", type=int, default=512)
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--big", type=int, default=3000)
    ap.add_argument("--big-loops", type=int, default=5)
    ap.add_argument("--small", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=2400000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A

    distinct = [GR._scene((100 + s, a.vertices, a.loops, 1.5)) for s in range(16)]
    big = GR._scene((200, a.big, a.big_loops, 2.0))
    small = GR._scene((300, a.small, 1, 1.1))
    results = [compare(A, torch, "batch", [distinct[g % 16] for g in range(a.graphs)], a.graphs, a.iterations, a.reps, a.warmup),
               compare(A, torch, "big", [big], 1, a.iterations, a.reps, a.warmup),
               compare(A, torch, "small", [small], 1, a.iterations, a.reps, a.warmup),
               correction(A, torch, a.points, a.reps, a.warmup)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/sgraph_rate.py", device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
