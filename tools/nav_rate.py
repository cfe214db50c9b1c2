#!/usr/bin/env python3
"""Rate of the path-planning stage (aria_nav_update_from_volume_device, aria_nav_solve_device, aria_nav_trace_device) at the
default 256 x 128 plane of the default 256 x 256 x 128 volume, with 256 goals and 4096 queries resident in HBM, timed with
HIP events on the handle's stream: 3 warm-up calls, then the median of 20. The volume is synthetic: every voxel of the band
seen and free, except rooms' walls with doors and a few pillars, which are solid.

Measured, each call on its own:
  update   rules 2-5: the band of the volume collapsed into cells, clearance, costs and move bits;
  solve    rule 6 for the 256 goals, one workgroup per goal, with the relaxation rounds the slowest goal needed and the
           time per goal;
  trace    rule 7 for the 4096 queries.
With --schedule-ab (needs the variants build, which knows ARIA_NAV_SCHEDULE) a second handle solves with the plainest
schedule, in-place all-cell sweeps in HBM, alternating with the shipped one inside one run, so that the gain of the shipped
schedule is a measured ratio. Both handles' fields are compared bitwise, and two fields against the restatement. There is no
pass or fail on time. Prints a table and writes one JSON line per measurement to --out.

Usage: nav_rate.py [--goals 256] [--queries 4096] [--reps 20] [--warmup 3] [--schedule-ab] [--out profiles/nav_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_volume(cfg):
    """VOXEL_DTYPE [nz, ny, nx]: the band seen and free; walls every 32 cells along x and z with a 12-cell door each (the default block_d2 = 16 keeps 4 cells off every wall), and pillars."""
    from aria_slam_amd.tsdf_ref import VOXEL_DTYPE
    nx, ny, nz = cfg.dims
    solid = np.zeros((nz, nx), bool)
    rng = np.random.default_rng(7)
    for x in range(32, nx, 32):
        solid[:, x] = True
        for z0 in range(0, nz, 32):
            d = z0 + int(rng.integers(4, 16))
            solid[d:d + 12, x] = False
    for z in range(32, nz, 32):
        solid[z, :] |= True
        for x0 in range(0, nx, 32):
            d = x0 + int(rng.integers(4, 16))
            solid[z, d:d + 12] = False
    for _ in range(24):
        x, z = int(rng.integers(2, nx - 4)), int(rng.integers(2, nz - 4))
        solid[z:z + 2, x:x + 2] = True
    vol = np.zeros((nz, ny, nx), VOXEL_DTYPE)
    b0, b1 = cfg.band
    vol["weight"][:, b0:b1, :] = 4
    vol["tsdf"][:, b0:b1, :] = np.where(solid, np.float32(-0.5), np.float32(0.5))[:, None, :]
    return vol


def timed(torch, stream, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=256)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--schedule-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_rate.json"))
    a = ap.parse_args()
    if a.schedule_ab:
        os.environ["ARIA_ORB_HIP_LIBRARY"] = os.path.join(ROOT, "aria_slam_amd", "libaria_orb_hip_variants.so")
        assert os.path.exists(os.environ["ARIA_ORB_HIP_LIBRARY"]), "--schedule-ab needs `make -C aria_slam_amd/csrc variants`"
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import nav_ref as R
    assert torch.cuda.is_available(), "nav_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    cfg = R.config()
    nu, nv = R.grid_shape(cfg)
    vol = synthetic_volume(cfg)
    cells = R.cells_from_volume(vol, cfg)
    d2, cost = R.build(cells, cfg)
    vfree, ufree = np.nonzero(cost != R.BLOCKED)
    rng = np.random.default_rng(11)
    G, Q, cap = a.goals, a.queries, 1024
    pick = rng.choice(len(ufree), G, replace=False)
    goals = np.stack([ufree[pick], vfree[pick]], axis=1).astype(np.int32)
    pick = rng.integers(0, len(ufree), Q)
    queries = np.stack([ufree[pick], vfree[pick], rng.integers(0, G, Q)], axis=1).astype(np.int32)
    with torch.cuda.stream(stream):
        d_vol = torch.from_numpy(vol.view(np.uint8).reshape(-1)).to(dev)
        d_goals, d_queries = torch.from_numpy(goals).to(dev), torch.from_numpy(queries).to(dev)
        d_rec = torch.zeros(Q * 16, dtype=torch.uint8, device=dev)
        d_paths = torch.zeros(Q * cap, dtype=torch.int32, device=dev)
    stream.synchronize()
    handles = {"sweeps": A.HipPathPlanner(stream=stream.cuda_stream)}
    if a.schedule_ab:
        os.environ["ARIA_NAV_SCHEDULE"] = "plain"
        handles["plain"] = A.HipPathPlanner(stream=stream.cuda_stream)
        del os.environ["ARIA_NAV_SCHEDULE"]
    times = {(name, what): [] for name in handles for what in ("update", "solve", "trace")}
    calls = {"update": lambda h: h.update(d_vol), "solve": lambda h: h.solve_device(d_goals, G),
             "trace": lambda h: h.trace_device(d_queries, Q, d_rec, d_paths, cap)}
    for rep in range(a.warmup + a.reps):
        for name, h in handles.items():                              # alternating: both schedules see the same clocks and caches
            for what in ("update", "solve", "trace"):
                ms = timed(torch, stream, lambda: calls[what](h))
                if rep >= a.warmup:
                    times[(name, what)].append(ms)
    results, fields = [], {}
    for name, h in handles.items():
        status = h.status()
        assert status in (0, -5), "deferred error %d" % status       # -5: a path longer than the tool's path_cap
        rounds = h.rounds(G)
        fields[name] = [h.field(g) for g in range(min(G, 8))]
        rec = d_rec.cpu().numpy().view(R.RECORD_DTYPE)
        for what in ("update", "solve", "trace"):
            t = times[(name, what)]
            res = dict(stage=what, schedule=name, plane=[nu, nv], goals=G, queries=Q, ms_median=float(np.median(t)), ms_min=float(np.min(t)),
                       ms_max=float(np.max(t)))
            if what == "solve":
                res.update(rounds_max=int(rounds.max()), rounds_median=float(np.median(rounds)), us_per_goal=res["ms_median"] * 1e3 / G)
            if what == "trace":
                res.update(ok=int((rec["status"] == 0).sum()), unreachable=int((rec["status"] == 1).sum()),
                           truncated=int((rec["status"] == 3).sum()), cells_max=int(rec["n_cells"].max()))
            results.append(res)
            print("%-7s %-7s %9.3f ms (min %.3f max %.3f) %s" % (name, what, res["ms_median"], res["ms_min"], res["ms_max"],
                                                                 {k: v for k, v in res.items() if k not in ("stage", "schedule", "ms_median", "ms_min", "ms_max", "plane", "goals", "queries")}))
    assert handles["sweeps"].cells().tobytes() == cells.tobytes() and handles["sweeps"].costs().tobytes() == cost.tobytes()
    for g in range(min(G, 2)):
        assert fields["sweeps"][g].tobytes() == R.field(cost, goals[g]).tobytes(), "field %d differs from the restatement" % g
    if a.schedule_ab:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(fields["sweeps"], fields["plain"])), "the schedules disagree"
        s = {r["schedule"]: r for r in results if r["stage"] == "solve"}
        print("solve, plain all-cell sweeps in HBM vs shipped: %.2fx (%d vs %d rounds at most)"
              % (s["plain"]["ms_median"] / s["sweeps"]["ms_median"], s["plain"]["rounds_max"], s["sweeps"]["rounds_max"]))
    for h in handles.values():
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
