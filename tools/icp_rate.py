#!/usr/bin/env python3
"""Rate of frame-to-model tracking (aria_icp_track_batch_device) with the default levels (strides 4, 2, 1 with 4, 5, 10
iterations: 19 x (accumulate, solve) per call), timed with HIP events on the handle's stream: 3 warm-up calls, then the median
of 20. Everything is made on the device: the default volume (256 x 256 x 128 voxels of 0.05 m) is filled from
tools/tsdf_rate.py's synthetic room along an arc of 32 poses; the model views are aria_ray_cast_batch_device at those poses
(depth and normals), and the live depth maps are casts 0.02 m and 0.01 rad further on, so every frame has a real step to find
and none stops early by eps in its first iterations.

Shapes: 1 frame of 752 x 480, 32 frames of 752 x 480, 256 frames of 640 x 480 (the 32 views eight times over).

Measured, alternating within one run so that clocks and cache state are shared (needs the variants build, which knows
ARIA_ICP_SCHEDULE; with the product library the shipped schedule alone is timed):
  shipped  four pixels per lane: a wave commits 29 int64 atomics per 256 level pixels;
  plain    one pixel per lane: the same commit per 64 level pixels.
Both handles' poses and records are compared byte for byte before anything is timed. The cast of the same model views (depth
and normal planes) is timed in the same run for scale. "hbm_share" is aria_icp_algorithmic_bytes over the time, as a share of
8 TB/s: the bytes of every iteration of every level as if no frame stopped early, an upper bound of the traffic.
Prints a table and writes one JSON line per measurement to --out.

Usage: icp_rate.py [--reps 20] [--warmup 3] [--out profiles/icp_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_rate   # noqa: E402

SHAPES = ((752, 480, 1), (752, 480, 32), (640, 480, 256))
N_POSES = 32


def step_on(ext, dyaw=0.01, dx=0.02):
    """The poses a little further along: turned by dyaw about y and moved by dx along the camera's x."""
    c, s = np.cos(dyaw), np.sin(dyaw)
    D = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    out = np.zeros_like(ext)
    for k in range(len(ext)):
        e = ext[k].reshape(3, 4)
        out[k] = np.concatenate([D @ e[:, :3], (D @ e[:, 3] + np.array([dx, 0.0, 0.0]))[:, None]], axis=1).reshape(12)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_rate.json"))
    a = ap.parse_args()
    variants = os.path.join(ROOT, "aria_slam_amd", "libaria_orb_hip_variants.so")
    if os.path.exists(variants) and not os.environ.get("ARIA_ORB_HIP_LIBRARY"):
        os.environ["ARIA_ORB_HIP_LIBRARY"] = variants
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import icp_ref, tsdf_ref
    assert torch.cuda.is_available(), "icp_rate.py measures on the GPU; there is no CPU fallback"
    ab = A.library_path().endswith("libaria_orb_hip_variants.so")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ext = tsdf_rate.trajectory(N_POSES)
    depths = np.stack([tsdf_rate.render(ext[k], tsdf_ref.EUROC_K) for k in range(N_POSES)])
    with torch.cuda.stream(stream):
        d_depth_in, d_ext32 = torch.from_numpy(depths).to(dev), torch.from_numpy(ext).to(dev)
    stream.synchronize()
    vol = A.HipTsdfVolume(stream=stream.cuda_stream)
    vol.integrate_batch_device(d_depth_in, tsdf_rate.W, tsdf_rate.H, d_ext32, N_POSES)
    vol.check()
    ray = A.HipVolumeRenderer.from_volume(vol, stream=stream.cuda_stream)
    os.environ.pop("ARIA_ICP_SCHEDULE", None)
    handles = {"shipped": A.HipDenseTracker.from_renderer(ray, tsdf_ref.EUROC_K, stream=stream.cuda_stream)}
    if ab:
        os.environ["ARIA_ICP_SCHEDULE"] = "plain"
        handles["plain"] = A.HipDenseTracker.from_renderer(ray, tsdf_ref.EUROC_K, stream=stream.cuda_stream)
        del os.environ["ARIA_ICP_SCHEDULE"]
    cfg = handles["shipped"].ref_config
    results = []
    for W, H, n in SHAPES:
        px = W * H
        tm = np.tile(ext, ((n + N_POSES - 1) // N_POSES, 1))[:n]
        with torch.cuda.stream(stream):
            d_tm, d_tl = torch.from_numpy(np.ascontiguousarray(tm)).to(dev), torch.from_numpy(step_on(tm)).to(dev)
            d_model = torch.zeros(n * px, dtype=torch.float32, device=dev)
            d_normal = torch.zeros(3 * n * px, dtype=torch.float32, device=dev)
            d_live = torch.zeros(n * px, dtype=torch.float32, device=dev)
            out = {k: (torch.zeros(12 * n, dtype=torch.float64, device=dev), torch.zeros(32 * n, dtype=torch.uint8, device=dev)) for k in handles}
        stream.synchronize()
        ray.cast_batch_device(d_tl, n, W, H, d_depth=d_live)
        cast = lambda: ray.cast_batch_device(d_tm, n, W, H, d_depth=d_model, d_normal=d_normal)   # noqa: E731
        cast()
        ray.check()

        def track(k):
            handles[k].track_batch_device(d_live, d_model, d_normal, d_tm, d_tm, n, W, H, d_extrinsics_out=out[k][0], d_results=out[k][1])

        for k in handles:
            track(k)
            handles[k].check()
        for k in handles:
            assert torch.equal(out[k][0], out["shipped"][0]) and torch.equal(out[k][1], out["shipped"][1]), "schedules differ"
        recs = out["shipped"][1].cpu().numpy().view(icp_ref.RESULT_DTYPE)
        for _ in range(a.warmup):
            cast()
            for k in handles:
                track(k)
        times = {k: [] for k in handles}
        t_cast = []
        for _ in range(a.reps):                                      # alternating: every form sees the same clocks and caches
            t_cast.append(tsdf_rate.timed(torch, stream, cast))
            for k in handles:
                times[k].append(tsdf_rate.timed(torch, stream, lambda: track(k)))
        ray.check()
        nbytes = handles["shipped"].algorithmic_bytes(W, H, n)
        assert nbytes == icp_ref.algorithmic_bytes(cfg, W, H, n)
        ms_cast = float(np.median(t_cast))
        results.append(dict(stage="cast_model", width=W, height=H, frames=n, ms_median=ms_cast, ms_min=float(np.min(t_cast)),
                            ms_max=float(np.max(t_cast)), us_per_frame=ms_cast * 1e3 / n))
        print("cast  %dx%d x %3d views (depth + normal)  %8.3f ms  %8.1f us/view" % (W, H, n, ms_cast, ms_cast * 1e3 / n))
        for k in handles:
            handles[k].check()
            ms = float(np.median(times[k]))
            res = dict(stage="track", schedule=k, width=W, height=H, frames=n, iterations=int(sum(cfg.iterations)), ms_median=ms,
                       ms_min=float(np.min(times[k])), ms_max=float(np.max(times[k])), us_per_frame=ms * 1e3 / n,
                       algorithmic_bytes=int(nbytes), hbm_share=nbytes / (ms * 1e-3) / tsdf_rate.HBM_PEAK,
                       valid_share=float(recs["valid"].mean()), iterations_run_mean=float(recs["iterations_run"].mean()),
                       n_corr_mean=float(recs["n_corr"].mean()), track_over_cast=ms / ms_cast)
            results.append(res)
            print("track %dx%d x %3d frames %-7s %8.3f ms (min %.3f max %.3f) %8.1f us/frame | %.2f%% of 8 TB/s | %.2fx the cast | valid %.2f, "
                  "%.1f iterations, %.0f correspondences" % (W, H, n, k, ms, res["ms_min"], res["ms_max"], res["us_per_frame"],
                                                             100 * res["hbm_share"], res["track_over_cast"], res["valid_share"],
                                                             res["iterations_run_mean"], res["n_corr_mean"]))
        if ab:
            print("  plain / shipped at %d frames: %.2fx" % (n, np.median(times["plain"]) / np.median(times["shipped"])))
        del d_model, d_normal, d_live
    for h in handles.values():
        h.close()
    ray.close()
    vol.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
