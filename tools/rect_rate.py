#!/usr/bin/env python3
"""Rate of the rectification stage's hot path (aria_rect_remap_batch_device): 4096 images at 752x480 and at 640x480 by
default, every one a distinct uniform-noise source image in HBM (2 x 1.5 GB at 752x480: far beyond the 256 MiB last-level
cache), through the left camera's map of the EuRoC MH stereo calibration (scaled to the shape), timed with HIP events on the
handle's stream. Prints microseconds per image and the fraction of 8 TB/s on the algorithmic 2 W H bytes, and one JSON line
per shape.

With the variants library (libaria_orb_hip_variants.so: built here when it is missing) it also prints two A/Bs, every form
in the same process and alternating, each checked bitwise against the shipped form's output:
  frame group   G = 1 (every frame re-reads its 4 B / pixel of map) against the shipped G: what amortising the map buys
  read form     the shipped three 8-byte row loads per lane against two unaligned 16-bit global loads per pixel
                (ARIA_RECT_READ=taps) and against the LDS-staged bounding box (ARIA_RECT_READ=lds)

--model kb4 runs all of it through the fisheye model: the EuRoC rig's two T_BS with the intrinsics and k1..k4 of a 190-degree
lens (TUM-VI's cam0, 512x512) scaled to the shape. The remap kernel does not know the model; the two figures that do are
printed for either model, per shape, from the product form alone:
  map build     wall-clock time of creating the handle (both cameras' maps built on the device, synchronised), median of 7
  points        aria_rect_points_batch_device over 4096 frames x 2000 keypoints uniform over the raw image, HIP events

This comparison is against the shipped form's output on this tool's own shapes; that every form equals the restatement on the
cases that reach each read form, frame group and limit is tools/rect_check.py (tests/test_gpu_rectify_variants.py).

Usage: rect_rate.py [--images 4096] [--shapes 752x480,640x480] [--reps 10] [--groups 1] [--no-ab] [--model radtan|kb4]
                    [--point-frames 4096] [--keypoints 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12   # B/s, the MI355X's HBM3E specification


# TUM-VI cam0 (512x512, equidistant): the intrinsics of --model kb4, on the EuRoC rig's extrinsics
KB4_K, KB4_D, KB4_SIZE = (190.978, 190.973, 254.931, 256.897), (0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673), (512, 512)


def calibration(W, H, model):
    from aria_slam_amd import rectify_ref as R
    if model == "kb4":
        return R.scaled_calibration(W, H, dict(R.EUROC_MH, K_l=KB4_K, K_r=KB4_K, D_l=KB4_D, D_r=KB4_D, size=KB4_SIZE))
    return R.scaled_calibration(W, H, R.EUROC_MH)


def make_rectifier(A, W, H, stream, env=None, model="radtan"):
    cal = calibration(W, H, model)
    for k in ("ARIA_RECT_GROUP", "ARIA_RECT_READ"):
        os.environ.pop(k, None)
    os.environ.update(env or {})                                  # read by aria_rect_create in the variants build only
    r = A.HipRectifier.from_stereo_calibration(cal["K_l"], cal["D_l"], cal["T_BS_l"], cal["K_r"], cal["D_r"], cal["T_BS_r"], (W, H),
                                               stream=stream.cuda_stream, model=model)
    for k in (env or {}):
        os.environ.pop(k, None)
    return r


def measure_model_stages(A, torch, W, H, model, frames, keypoints, reps, warmup):
    """The two figures that depend on the distortion model: handle creation (the map build) and the points batch."""
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    create = []
    for _ in range(7 + 1):                                        # the first creation loads the code object: dropped
        t = time.perf_counter()
        r = make_rectifier(A, W, H, stream, model=model)
        create.append((time.perf_counter() - t) * 1e3)
        r.close()
    create = create[1:]
    r = make_rectifier(A, W, H, stream, model=model)
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=dev)
        gen.manual_seed(8)
        kp = torch.zeros((frames, keypoints, 6), dtype=torch.float32, device=dev)
        kp[:, :, 0] = torch.rand((frames, keypoints), device=dev, generator=gen) * (W - 1)
        kp[:, :, 1] = torch.rand((frames, keypoints), device=dev, generator=gen) * (H - 1)
        out = torch.zeros_like(kp)
        counts = torch.full((frames,), keypoints, dtype=torch.int32, device=dev)
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):
        t0.record(stream)
        r.points_batch_device(kp, counts, keypoints, frames, out)
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    r.check()
    with torch.cuda.stream(stream):
        moved = float(((out[:, :, 0] != -1) | (out[:, :, 1] != -1)).float().mean())
    stream.synchronize()
    r.close()
    ms = float(np.median(times))
    res = dict(model=model, width=W, height=H, create_ms_median=float(np.median(create)), create_ms_min=float(np.min(create)),
               create_ms_max=float(np.max(create)), point_frames=frames, keypoints=keypoints, points_ms_median=ms,
               points_ms_min=float(np.min(times)), points_ms_max=float(np.max(times)),
               points_ns_per_keypoint=ms * 1e6 / (frames * keypoints), points_valid_share=moved)
    print("%dx%d, %s: handle creation (two maps built) %.3f ms (median of %d, min %.3f max %.3f); points, %d frames x %d keypoints: "
          "%.3f ms (median of %d, min %.3f max %.3f) = %.3f ns/keypoint, %.1f %% valid"
          % (W, H, model, res["create_ms_median"], len(create), res["create_ms_min"], res["create_ms_max"], frames, keypoints, ms, reps,
             res["points_ms_min"], res["points_ms_max"], res["points_ns_per_keypoint"], 100 * moved))
    print(json.dumps(res))
    return res


def measure(A, torch, W, H, B, reps, warmup, ab, groups=(1,), model="radtan"):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        src = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device=dev, generator=gen)
        dst = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
        other = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
    stream.synchronize()
    forms = [("shipped", None)]
    if ab:
        forms += [("G=%d" % g, {"ARIA_RECT_GROUP": str(g)}) for g in groups]
        forms += [("taps", {"ARIA_RECT_READ": "taps"}), ("lds", {"ARIA_RECT_READ": "lds"})]
    rect = [(name, make_rectifier(A, W, H, stream, env, model)) for name, env in forms]
    times = {name: [] for name, _ in rect}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, r in rect:                                          # warm-up, and every form against the shipped one's bytes
        out = dst if name == "shipped" else other
        for _ in range(warmup):
            r.remap_batch_device(src, B, out)
        r.check()
        if name != "shipped":
            with torch.cuda.stream(stream):
                same = bool(torch.equal(dst, other))
            stream.synchronize()
            assert same, "%s differs from the shipped form" % name
    for _ in range(reps):                                         # alternating
        for name, r in rect:
            t0.record(stream)
            r.remap_batch_device(src, B, dst if name == "shipped" else other)
            t1.record(stream)
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    invalid = float((rect[0][1].map(0) == 0xFFFFFFFF).mean())
    res = dict(model=model, width=W, height=H, images=B, reps=reps, invalid_share=invalid, algorithmic_bytes_per_image=2 * W * H)
    for name, r in rect:
        ms = float(np.median(times[name]))
        us = ms * 1e3 / B
        frac = 2.0 * W * H / (us * 1e-6) / PEAK
        key = name.replace(" ", "_").replace("=", "")
        res[key + "_ms_median"], res[key + "_ms_min"], res[key + "_ms_max"] = ms, float(np.min(times[name])), float(np.max(times[name]))
        res[key + "_us_per_image"], res[key + "_fraction_of_8TBps"] = us, frac
        print("%dx%d, %d images, %-8s %.3f ms (median of %d, min %.3f max %.3f) = %.3f us/image = %.1f %% of 8 TB/s on 2WH bytes"
              % (W, H, B, name + ":", ms, reps, np.min(times[name]), np.max(times[name]), us, 100 * frac))
        r.close()
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--shapes", default="752x480,640x480")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", default="1", help="frame-group sizes of the A/B beside the shipped one")
    ap.add_argument("--no-ab", action="store_true", help="the product library alone: no frame-group and read-form A/B")
    ap.add_argument("--model", choices=("radtan", "kb4"), default="radtan")
    ap.add_argument("--point-frames", type=int, default=4096)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--no-remap", action="store_true", help="map build and points only")
    a = ap.parse_args()
    if not a.no_ab and not os.environ.get("ARIA_ORB_HIP_LIBRARY"):
        variants = os.path.join(ROOT, "aria_slam_amd", "libaria_orb_hip_variants.so")
        if not os.path.exists(variants):
            import subprocess
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "aria_slam_amd", "csrc"), "-s", "variants"])
        os.environ["ARIA_ORB_HIP_LIBRARY"] = variants             # read when aria_slam_amd._lib is imported
    import torch
    import aria_slam_amd as A
    assert torch.cuda.is_available(), "rect_rate.py measures on the GPU; there is no CPU fallback"
    for shape in a.shapes.split(","):
        W, H = (int(v) for v in shape.split("x"))
        if not a.no_remap:
            measure(A, torch, W, H, a.images, a.reps, a.warmup, not a.no_ab, [int(g) for g in a.groups.split(",")], a.model)
        measure_model_stages(A, torch, W, H, a.model, a.point_frames, a.keypoints, a.reps, a.warmup)


if __name__ == "__main__":
    main()
