#!/usr/bin/env python3
"""Rate of guided matching (aria_proj_search_batch_device: binning + projection + window search + uniqueness + compaction):
4096 frames x 2000 features at 752x480 against 2000 landmarks per frame by default, timed with HIP events on the handle's
stream. The keypoints and descriptors are what aria_orb_extract_batch_device leaves in HBM for 16 distinct synthetic frames,
tiled over the batch; the landmarks of a frame are its own keypoints back-projected at a depth pattern (one array of
16 x kp_stride records, a range per frame) and searched under a small motion, the tracking case.

The yardstick, in the same process on the same data: aria_matcher_match_batch_device (brute-force kNN-2 + ratio) of each
frame's descriptors against the next frame's -- the job this stage replaces for tracking.

Also the join aria_proj_landmarks_from_map_device over a map of about 2 M points (a synthetic two-view scene triangulated
--map-pairs times on the device). Prints one JSON line.

Usage: proj_rate.py [--frames 4096] [--shape 752x480x2000] [--reps 20] [--map-pairs 2048]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = 16


def timed(torch, stream, fn, check, reps, warmup):
    for _ in range(warmup):
        fn()
    check()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    check()
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def measure_search(A, torch, W, H, nf, B, reps, warmup):
    from aria_slam_amd import stereo_ref as SR
    from aria_slam_amd._lib import KP_DTYPE, PROJ_LANDMARK_DTYPE
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    imgs = np.stack([SR.stereo_pair(100 + s, W, H)[0] for s in range(DISTINCT)])
    with torch.cuda.stream(stream):
        d_img = torch.from_numpy(imgs).to(dev)
    stream.synchronize()
    ext = A.OrbHipExtractor(max_features=nf, stream=stream.cuda_stream, max_width=W, max_height=H, max_batch=DISTINCT)
    cap = ext.kp_capacity()
    with torch.cuda.stream(stream):
        k = torch.zeros((DISTINCT, cap, 24), dtype=torch.uint8, device=dev)
        d = torch.zeros((DISTINCT, cap, 32), dtype=torch.uint8, device=dev)
        c = torch.zeros((DISTINCT,), dtype=torch.int32, device=dev)
    stream.synchronize()
    ext.extract_batch_device(d_img, DISTINCT, W, H, k, d, c, cap)
    ext.check()
    ext.close()
    kp = k.cpu().numpy().reshape(-1).view(KP_DTYPE).reshape(DISTINCT, cap)
    desc, counts = d.cpu().numpy(), c.cpu().numpy()
    K = (458.654, 457.296, 367.215, 248.375)
    lm = np.zeros((DISTINCT, cap), PROJ_LANDMARK_DTYPE)
    lm["octave"] = -1
    for s in range(DISTINCT):
        n = counts[s]
        z = 2.0 + (np.arange(n) % 7)
        lm["X"][s, :n] = np.stack([(kp["x"][s, :n] - K[2]) / K[0] * z, (kp["y"][s, :n] - K[3]) / K[1] * z, z], axis=1)
        lm["desc"][s, :n], lm["octave"][s, :n], lm["source"][s, :n] = desc[s, :n], kp["octave"][s, :n], np.arange(n)
    ang = np.deg2rad(0.3)
    pose = np.array([np.cos(ang), 0, np.sin(ang), 0.01, 0, 1, 0, -0.005, -np.sin(ang), 0, np.cos(ang), 0.002])
    ranges = np.array([[(f % DISTINCT) * cap, cap] for f in range(B)], np.int32)
    reps_of = (B + DISTINCT - 1) // DISTINCT
    with torch.cuda.stream(stream):
        tile = lambda t: t.repeat((reps_of,) + (1,) * (t.dim() - 1))[:B].contiguous()   # noqa: E731
        kb, db, nb = tile(k), tile(d), tile(c)
        d_pose = torch.from_numpy(np.tile(pose, (B, 1))).to(dev)
        d_land = torch.from_numpy(lm.view(np.uint8).reshape(-1)).to(dev)
        d_range = torch.from_numpy(ranges.reshape(-1)).to(dev)
        obs = torch.zeros((B, cap, 24), dtype=torch.uint8, device=dev)
        corr = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
        pairs = torch.zeros((B, cap, 8), dtype=torch.uint8, device=dev)
        ncorr = torch.zeros((B,), dtype=torch.int32, device=dev)
        m = torch.zeros((B, cap, 12), dtype=torch.uint8, device=dev)
        nm = torch.zeros((B,), dtype=torch.int32, device=dev)
    stream.synchronize()
    pm = A.HipProjectionMatcher(K=K, stream=stream.cuda_stream)
    mat = A.HipMatcher(stream=stream.cuda_stream, max_query=max(cap, 4096), max_train=max(cap, 4096))

    def run_search():
        pm.search_batch_device(d_pose, kb, db, nb, cap, W, H, d_land, DISTINCT * cap, d_range, cap, B, obs, corr, pairs, ncorr)

    def run_brute():
        mat.match_batch_device(db.data_ptr() + cap * 32, nb.data_ptr() + 4, db, nb, B - 1, cap * 32, 0.75, m, nm, cap)

    ms, ms_min, ms_max = timed(torch, stream, run_search, pm.check, reps, warmup)
    bms, bms_min, bms_max = timed(torch, stream, run_brute, lambda: stream.synchronize(), reps, warmup)
    res = dict(width=W, height=H, features=nf, frames=B, kp_stride=cap, keypoints=float(counts.mean()), landmarks_per_frame=cap,
               matched_per_frame=float(ncorr.float().mean().item()), search_ms_median=ms, search_ms_min=ms_min, search_ms_max=ms_max,
               search_us_per_frame=ms * 1e3 / B, brute_matches_per_pair=float(nm[:B - 1].float().mean().item()), brute_ms_median=bms,
               brute_ms_min=bms_min, brute_ms_max=bms_max, brute_us_per_pair=bms * 1e3 / (B - 1))
    print("%dx%d / %d features, %d frames: guided search %.3f ms (median of %d, min %.3f max %.3f) = %.3f us/frame, %.0f of %.0f "
          "landmarks matched; brute-force kNN-2 + ratio %.3f ms (min %.3f max %.3f) = %.3f us/pair, %.0f matches"
          % (W, H, nf, B, ms, reps, ms_min, ms_max, res["search_us_per_frame"], res["matched_per_frame"], res["keypoints"], bms, bms_min,
             bms_max, res["brute_us_per_pair"], res["brute_matches_per_pair"]))
    pm.close()
    mat.close()
    return res


def measure_join(A, torch, map_pairs, reps, warmup):
    from aria_slam_amd import _lib
    from aria_slam_amd import pose_ref as P
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    K = P.EUROC_K
    rng = np.random.default_rng(7)
    n = 1024
    u, v, z = rng.uniform(60, 690, n), rng.uniform(40, 440, n), rng.uniform(3, 12, n)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    R2, t2 = P.rot([0, 1, 0], 4), np.array([1.0, 0.0, 0.0])
    Xc = X @ R2.T + t2
    kp = np.zeros((2, n), _lib.KP_DTYPE)
    kp["x"][0], kp["y"][0] = u, v
    kp["x"][1], kp["y"][1] = K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]
    kp["octave"][1] = rng.integers(0, 8, n)
    m = np.zeros(n, _lib.MATCH_DTYPE)
    m["query_idx"] = m["train_idx"] = np.arange(n)
    ext = np.concatenate([np.hstack([np.eye(3), np.zeros((3, 1))]).ravel(), np.hstack([R2, t2[:, None]]).ravel()])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    with torch.cuda.stream(stream):
        d_k1, d_k2 = up(np.tile(kp[0], map_pairs)), up(np.tile(kp[1], map_pairs))
        d_m, d_n = up(np.tile(m, map_pairs)), up(np.full(map_pairs, n, np.int32))
        d_ext = up(np.tile(ext, map_pairs))
        d_desc = torch.randint(0, 256, (map_pairs * n * 32,), dtype=torch.uint8, device=dev)
    stream.synchronize()
    mp = A.HipMapper(K=K, stream=stream.cuda_stream, capacity=map_pairs * n)
    pm = A.HipProjectionMatcher(K=K, stream=stream.cuda_stream)
    mp.triangulate_batch_device(d_k1, d_n, d_k2, d_n, n, d_m, d_n, map_pairs, n, d_extrinsics=d_ext, pair_base=0)
    mp.check()
    size = mp.size()
    with torch.cuda.stream(stream):
        d_land = torch.zeros((size * 64,), dtype=torch.uint8, device=dev)
        d_nl = torch.zeros((1,), dtype=torch.int32, device=dev)
    stream.synchronize()
    ms, ms_min, ms_max = timed(torch, stream, lambda: pm.landmarks_from_map_device(mp, 0, size, 0, 2, d_k2, d_desc, d_n, n, map_pairs,
                                                                                 d_land, d_nl), pm.check, reps, warmup)
    res = dict(join_points=size, join_ms_median=ms, join_ms_min=ms_min, join_ms_max=ms_max, join_ns_per_point=ms * 1e6 / max(size, 1),
               join_written=int(d_nl.item()))
    print("join: %d map points -> landmarks %.3f ms (min %.3f max %.3f) = %.2f ns/point" % (size, ms, ms_min, ms_max, res["join_ns_per_point"]))
    pm.close()
    mp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--shape", default="752x480x2000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--map-pairs", type=int, default=2048)
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    assert torch.cuda.is_available(), "proj_rate.py measures on the GPU; there is no CPU fallback"
    W, H, nf = (int(v) for v in a.shape.split("x"))
    res = measure_search(A, torch, W, H, nf, a.frames, a.reps, a.warmup)
    if a.map_pairs > 0:
        res.update(measure_join(A, torch, a.map_pairs, a.reps, a.warmup))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
