#!/usr/bin/env python3
"""Rate of the dense depth fusion stage (aria_tsdf_integrate_batch_device and aria_tsdf_extract_points_device) at the default
volume (256 x 256 x 128 voxels of 0.05 m) with 752x480 depth maps resident in HBM, timed with HIP events on the handle's
stream: 3 warm-up calls, then the median of 20. The depth maps are analytic renders of a wall and a sphere along a synthetic
trajectory of 32 poses (a sideways arc with a yaw sweep), with the left images' place taken by a gray ramp.

Measured, alternating within one run so that clocks and cache state are shared:
  one call      the 32 frames in one aria_tsdf_integrate_batch_device: every voxel record read and written once;
  32 calls      the same frames one per call: every record read and written 32 times (what keeping the voxel in registers buys);
  extraction    count, scan and emit into a buffer that holds every point.
With --cull-ab (needs the variants build, which knows ARIA_TSDF_CULL) a second handle walks every frame in every tile, for
the A/B of the frustum test. Prints a table and writes one JSON line per measurement to --out.

The "bound" column is an inference from the timing alone, not a measurement: a form that takes less than twice what its
algorithmic bytes take at the 8 TB/s HBM peak is called memory-bound, any other is not. No counters are read; launch overhead
(the 32-call form pays 96 launches) and traffic served from the Infinity Cache are not told apart.

Usage: tsdf_rate.py [--frames 32] [--reps 20] [--warmup 3] [--cull-ab] [--out profiles/tsdf_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
W, H = 752, 480
WALL_Z, SPHERE_C, SPHERE_R = 5.0, np.array([0.5, 0.2, 3.0]), 0.8


def trajectory(n):
    """n world-to-camera [R|t] records: the camera moves from x = -1.5 to +1.5 m and turns from +0.3 to -0.3 rad of yaw."""
    out = np.zeros((n, 12))
    for k in range(n):
        a = k / max(n - 1, 1)
        yaw, x = 0.3 - 0.6 * a, -1.5 + 3.0 * a
        c, s = np.cos(yaw), np.sin(yaw)
        Rcw = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
        out[k] = np.concatenate([Rcw, (-Rcw @ np.array([x, 0.0, 0.0]))[:, None]], axis=1).reshape(12)
    return out


def render(ext, K):
    """fp32 depth [H, W] of the wall z = WALL_Z and the sphere from one pose."""
    e = ext.reshape(3, 4)
    Rcw, t = e[:, :3], e[:, 3]
    o = -Rcw.T @ t
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], axis=-1) @ Rcw
    with np.errstate(all="ignore"):
        s = np.where(d[..., 2] > 1e-9, (WALL_Z - o[2]) / d[..., 2], np.inf)
        oc = o - SPHERE_C
        a, b, c = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        s1 = (-b - np.sqrt(disc)) / (2 * a)
        s = np.minimum(s, np.where((disc > 0) & (s1 > 0), s1, np.inf))
    return np.where(np.isfinite(s), s, 0.0).astype(np.float32)


def timed(torch, stream, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cull-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_rate.json"))
    a = ap.parse_args()
    if a.cull_ab:
        os.environ["ARIA_ORB_HIP_LIBRARY"] = os.path.join(ROOT, "aria_slam_amd", "libaria_orb_hip_variants.so")
        assert os.path.exists(os.environ["ARIA_ORB_HIP_LIBRARY"]), "--cull-ab needs `make -C aria_slam_amd/csrc variants`"
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import tsdf, tsdf_ref
    assert torch.cuda.is_available(), "tsdf_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n = a.frames
    ext = trajectory(n)
    depths = np.stack([render(ext[k], tsdf_ref.EUROC_K) for k in range(n)])
    gray = np.tile((np.arange(W) % 256).astype(np.uint8), (n, H, 1))
    with torch.cuda.stream(stream):
        d_depth, d_ext, d_img = (torch.from_numpy(x).to(dev) for x in (depths, ext, gray))
    stream.synchronize()
    handles = {"cull": A.HipTsdfVolume(stream=stream.cuda_stream)}
    if a.cull_ab:
        os.environ["ARIA_TSDF_CULL"] = "0"
        handles["no cull"] = A.HipTsdfVolume(stream=stream.cuda_stream)
        del os.environ["ARIA_TSDF_CULL"]
    nx, ny, nz = handles["cull"].dims
    results = []
    for name, h in handles.items():
        def one_call():
            h.integrate_batch_device(d_depth, W, H, d_ext, n, None, d_img)

        def many_calls():
            for k in range(n):
                h.integrate_batch_device(d_depth[k], W, H, d_ext[k], 1, None, d_img[k])

        for _ in range(a.warmup):
            one_call()
            many_calls()
        h.check()
        t_one, t_many = [], []
        for _ in range(a.reps):                                      # alternating: both forms see the same clocks and caches
            t_one.append(timed(torch, stream, one_call))
            t_many.append(timed(torch, stream, many_calls))
        h.check()
        total = h.count_points()
        with torch.cuda.stream(stream):
            d_pts = torch.zeros(max(total, 1) * 16, dtype=torch.uint8, device=dev)
            d_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        stream.synchronize()

        def extract():
            h.extract_points_device(d_pts, total, d_cnt)

        for _ in range(a.warmup):
            extract()
        t_ext = [timed(torch, stream, extract) for _ in range(a.reps)]
        h.check()
        assert int(d_cnt.item()) == total
        observed = int((h.voxels()["weight"] > 0).sum())
        for what, times, calls in (("one call", t_one, 1), ("%d calls" % n, t_many, n), ("extraction", t_ext, 1)):
            ms = float(np.median(times))
            if what == "extraction":
                alg = 8 * nx * ny * nz + 16 * total                 # every record read once, every point written once
            else:
                alg = calls * tsdf.algorithmic_bytes(nx, ny, nz, W, H, n // calls)
            floor_us = alg / HBM_PEAK * 1e6
            res = dict(stage=what, frustum_test=name, frames=n, width=W, height=H, dims=[nx, ny, nz], ms_median=ms,
                       ms_min=float(np.min(times)), ms_max=float(np.max(times)), us_per_frame=ms * 1e3 / n, algorithmic_bytes=alg,
                       us_at_hbm_peak=floor_us, algorithmic_share_of_hbm_peak=floor_us / (ms * 1e3),
                       ns_per_voxel_frame=ms * 1e6 / (nx * ny * nz * n) if what != "extraction" else None,
                       bound=("memory (inferred: under twice the HBM floor; no counters)" if ms * 1e3 < 2 * floor_us else
                              "not memory (inferred: over twice the HBM floor; no counters)"),
                       points=total, observed_voxels=observed)
            results.append(res)
            print("%-8s %-11s %8.3f ms (min %.3f max %.3f) %8.1f us/frame | %7.1f MB algorithmic = %6.1f us at 8 TB/s (%.1f %% of peak) | %s"
                  % (name, what, ms, res["ms_min"], res["ms_max"], res["us_per_frame"], alg / 1e6, floor_us,
                     100 * res["algorithmic_share_of_hbm_peak"], res["bound"]))
        print("%s: %d points, %d observed voxels" % (name, total, observed))
    ref = [r for r in results if r["frustum_test"] == "cull"]
    print("one call vs %d calls: %.2fx" % (n, ref[1]["ms_median"] / ref[0]["ms_median"]))
    for h in handles.values():
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
