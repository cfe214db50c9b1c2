#!/usr/bin/env python3
"""Rate of the ray casting stage (aria_ray_update_from_volume_device and aria_ray_cast_batch_device) at the default volume
(256 x 256 x 128 voxels of 0.05 m, 64 MiB of records), filled on the device from tools/tsdf_rate.py's synthetic room (a wall
and a sphere along an arc of 32 poses), timed with HIP events on the handle's stream: 3 warm-up calls, then the median of
20. Views of 752 x 480 and 640 x 480 at the trajectory's poses, batches of 1 and 32, all four planes and the view records.

Measured, alternating within one run so that clocks and cache state are shared:
  skip 1   the product: no record load in a brick of 8 x 8 x 8 voxels that holds no seen negative voxel;
  skip 0   every sample inside the volume loads its record.
Both handles read the same volume; their outputs are compared byte for byte before anything is timed. The update (the brick
words) is timed on its own. Prints a table and writes one JSON line per measurement to --out.

"samples" is the definition's count, width x height x n_steps per view, an upper bound: the kernel clips each ray to the
volume's box and stops at its hit, and no counter of the samples it actually takes is read. The per-sample figure is therefore
time per DEFINED sample, good for comparing the two settings, not a cost per loop iteration.

Usage: ray_rate.py [--views 32] [--reps 20] [--warmup 3] [--out profiles/ray_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_rate   # noqa: E402

SIZES = ((752, 480), (640, 480))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_rate.json"))
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import ray_ref, render, tsdf_ref
    assert torch.cuda.is_available(), "ray_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n = a.views
    ext = tsdf_rate.trajectory(n)
    depths = np.stack([tsdf_rate.render(ext[k], tsdf_ref.EUROC_K) for k in range(n)])
    gray = np.tile((np.arange(tsdf_rate.W) % 256).astype(np.uint8), (n, tsdf_rate.H, 1))
    with torch.cuda.stream(stream):
        d_depth_in, d_ext, d_img = (torch.from_numpy(x).to(dev) for x in (depths, ext, gray))
    stream.synchronize()
    vol = A.HipTsdfVolume(stream=stream.cuda_stream)
    vol.integrate_batch_device(d_depth_in, tsdf_rate.W, tsdf_rate.H, d_ext, n, None, d_img)
    vol.check()
    handles = {s: A.HipVolumeRenderer.from_volume(vol, skip=s, stream=stream.cuda_stream) for s in (1, 0)}
    steps = ray_ref.n_steps(handles[1].ref_config)
    nx, ny, nz = vol.dims
    results = []

    t_upd = []
    for _ in range(a.warmup):
        handles[1].update(vol)
    for _ in range(a.reps):
        t_upd.append(tsdf_rate.timed(torch, stream, lambda: handles[1].update(vol)))
    handles[1].check()
    ms = float(np.median(t_upd))
    results.append(dict(stage="update", dims=[nx, ny, nz], ms_median=ms, ms_min=float(np.min(t_upd)), ms_max=float(np.max(t_upd)),
                        record_bytes=8 * nx * ny * nz, us_at_hbm_peak=8 * nx * ny * nz / tsdf_rate.HBM_PEAK * 1e6))
    print("update   %8.3f ms (min %.3f max %.3f) | %d MiB of records read once = %.1f us at 8 TB/s"
          % (ms, results[-1]["ms_min"], results[-1]["ms_max"], (8 * nx * ny * nz) >> 20, results[-1]["us_at_hbm_peak"]))

    for W, H in SIZES:
        px = W * H
        with torch.cuda.stream(stream):
            out = {s: dict(depth=torch.zeros(n * px, dtype=torch.float32, device=dev), normal=torch.zeros(3 * n * px, dtype=torch.float32, device=dev),
                           gray=torch.zeros(n * px, dtype=torch.uint8, device=dev), shade=torch.zeros(n * px, dtype=torch.uint8, device=dev),
                           views=torch.zeros(16 * n, dtype=torch.uint8, device=dev)) for s in (1, 0)}
        stream.synchronize()

        def cast(s, batch):
            o = out[s]
            handles[s].cast_batch_device(d_ext, batch, W, H, d_depth=o["depth"], d_normal=o["normal"], d_gray=o["gray"], d_shade=o["shade"],
                                         d_views=o["views"])

        for s in (1, 0):
            cast(s, n)
            handles[s].check()
        for k in out[1]:
            assert torch.equal(out[1][k], out[0][k]), "skip 1 and skip 0 differ in " + k
        views = out[1]["views"].cpu().numpy().view(ray_ref.VIEW_DTYPE)
        hit_share = float(views["n_hit"].sum()) / (n * px)
        for batch in (1, n):
            for _ in range(a.warmup):
                cast(1, batch)
                cast(0, batch)
            times = {1: [], 0: []}
            for _ in range(a.reps):                                  # alternating: both settings see the same clocks and caches
                for s in (1, 0):
                    times[s].append(tsdf_rate.timed(torch, stream, lambda: cast(s, batch)))
            for s in (1, 0):
                handles[s].check()
                ms = float(np.median(times[s]))
                samples = px * steps * batch
                res = dict(stage="cast", skip=s, width=W, height=H, views=batch, n_steps=steps, ms_median=ms, ms_min=float(np.min(times[s])),
                           ms_max=float(np.max(times[s])), us_per_view=ms * 1e3 / batch, defined_samples=samples,
                           ps_per_defined_sample=ms * 1e9 / samples, bytes_written=render.algorithmic_bytes(W, H, batch),
                           hit_share=hit_share)
                results.append(res)
                print("cast %dx%d x %2d views skip %d %8.3f ms (min %.3f max %.3f) %8.1f us/view | %.1f ps per defined sample | hit share %.3f"
                      % (W, H, batch, s, ms, res["ms_min"], res["ms_max"], res["us_per_view"], res["ps_per_defined_sample"], hit_share))
            print("  skip 0 / skip 1 at %d views: %.2fx" % (batch, np.median(times[0]) / np.median(times[1])))
    for h in handles.values():
        h.close()
    vol.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
