#!/usr/bin/env python3
"""Rate of the mesh stage (aria_mesh_update_from_volume_device and aria_mesh_extract_device) at the default volume
(256 x 256 x 128 voxels of 0.05 m) after the scene of tools/tsdf_rate.py has been integrated: 32 analytic 752x480 depth maps
of a wall and a sphere along its synthetic trajectory. Timed with HIP events on the handles' stream with nothing else on it:
3 warm-up calls, then the median of 20.

Measured, alternating within one run so that clocks and cache state are shared:
  update            k_mesh_count: every record read once, a word per voxel written;
  extract           k_mesh_scan and k_mesh_emit into buffers that hold the whole mesh;
  update + extract  both, the figure a caller who meshes a changed volume pays;
  points            aria_tsdf_extract_points_device of the same volume (count, scan, emit): orientation, not a threshold.
Prints a table and writes one JSON line per measurement to --out.

The "bound" column is an inference from the timing alone, not a measurement: a form that takes less than twice what its
algorithmic bytes take at the 8 TB/s HBM peak is called memory-bound, any other is not. No counters are read; the 64 MiB volume
fits the Infinity Cache, and traffic served from there is not told apart from HBM traffic.

Usage: mesh_rate.py [--frames 32] [--reps 20] [--warmup 3] [--out profiles/mesh_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tsdf_rate import HBM_PEAK, H, W, render, timed, trajectory   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_rate.json"))
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import mesh, tsdf_ref
    assert torch.cuda.is_available(), "mesh_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n = a.frames
    ext = trajectory(n)
    depths = np.stack([render(ext[k], tsdf_ref.EUROC_K) for k in range(n)])
    gray = np.tile((np.arange(W) % 256).astype(np.uint8), (n, H, 1))
    with torch.cuda.stream(stream):
        d_depth, d_ext, d_img = (torch.from_numpy(x).to(dev) for x in (depths, ext, gray))
    stream.synchronize()
    vol = A.HipTsdfVolume(stream=stream.cuda_stream)
    vol.integrate_batch_device(d_depth, W, H, d_ext, n, None, d_img)
    vol.check()
    nx, ny, nz = vol.dims
    h = A.HipVolumeMesher.from_volume(vol, stream=stream.cuda_stream)
    nv, nt = h.count()
    points = vol.count_points()
    with torch.cuda.stream(stream):
        d_v = torch.zeros(max(nv, 1) * 16, dtype=torch.uint8, device=dev)
        d_t = torch.zeros(max(nt, 1) * 12, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(2, dtype=torch.int64, device=dev)
        d_pts = torch.zeros(max(points, 1) * 16, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    stream.synchronize()

    def update():
        h.update(vol.device_voxels())

    def extract():
        h.extract_device(d_v, nv, d_t, nt, d_n)

    def both():
        update()
        extract()

    def extract_points():
        vol.extract_points_device(d_pts, points, d_cnt)

    forms = (("update", update), ("extract", extract), ("update + extract", both), ("points", extract_points))
    for _ in range(a.warmup):
        for _, fn in forms:
            fn()
    h.check()
    vol.check()
    times = {name: [] for name, _ in forms}
    for _ in range(a.reps):                                          # alternating: every form sees the same clocks and caches
        for name, fn in forms:
            times[name].append(timed(torch, stream, fn))
    h.check()
    vol.check()
    assert tuple(int(v) for v in d_n.cpu()) == (nv, nt) and int(d_cnt.item()) == points
    n_vox = nx * ny * nz
    out_bytes = 16 * nv + 12 * nt
    alg = {"update": 12 * n_vox, "extract": 4 * n_vox + out_bytes, "update + extract": mesh.algorithmic_bytes(nx, ny, nz, nv, nt),
           "points": 8 * n_vox + 16 * points}
    results = []
    for name, _ in forms:
        ms = float(np.median(times[name]))
        floor_us = alg[name] / HBM_PEAK * 1e6
        res = dict(stage=name, frames=n, dims=[nx, ny, nz], ms_median=ms, ms_min=float(np.min(times[name])),
                   ms_max=float(np.max(times[name])), algorithmic_bytes=alg[name], us_at_hbm_peak=floor_us,
                   algorithmic_share_of_hbm_peak=floor_us / (ms * 1e3),
                   bound=("memory (inferred: under twice the HBM floor; no counters)" if ms * 1e3 < 2 * floor_us else
                          "not memory (inferred: over twice the HBM floor; no counters)"),
                   vertices=nv, triangles=nt, points=points, scratch_bytes=mesh.scratch_bytes(nx, ny, nz))
        results.append(res)
        print("%-17s %8.1f us (min %.1f max %.1f) | %7.1f MB algorithmic = %6.1f us at 8 TB/s (%.1f %% of peak) | %s"
              % (name, ms * 1e3, res["ms_min"] * 1e3, res["ms_max"] * 1e3, alg[name] / 1e6, floor_us,
                 100 * res["algorithmic_share_of_hbm_peak"], res["bound"]))
    print("%d vertices, %d triangles, %d surface points" % (nv, nt, points))
    h.close()
    vol.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
