#!/usr/bin/env python3
"""Rate of the sparse stereo stage (aria_stereo_match_batch_device: candidates + SAD slide + sub-pixel + median filter, and
aria_stereo_scale_batch_device): 4096 rectified pairs at 640x480 / 2000 features and at 752x480 / 1000 features by default,
timed with HIP events on the handle's stream. The inputs are what aria_orb_extract_batch_device leaves in HBM for 16 distinct
synthetic pairs (stereo_ref.stereo_pair: row disparities 7, 19.5 and 42.25 px), tiled over the batch on the device -- every
pair has its own images, keypoints and descriptors in memory. Prints microseconds per pair and one JSON line per shape.

Usage: stereo_rate.py [--pairs 4096] [--shapes 640x480x2000,752x480x1000] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = 16


def measure(A, torch, W, H, nf, B, reps, warmup):
    from aria_slam_amd import stereo_ref as R
    from aria_slam_amd._lib import MATCH_DTYPE, POSE_RESULT_DTYPE
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    pairs = [R.stereo_pair(100 + s, W, H) for s in range(DISTINCT)]
    with torch.cuda.stream(stream):
        left = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
        right = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    stream.synchronize()
    ext = A.OrbHipExtractor(max_features=nf, stream=stream.cuda_stream, max_width=W, max_height=H, max_batch=DISTINCT)
    cap = ext.kp_capacity()
    side = []
    for img in (left, right):
        with torch.cuda.stream(stream):
            k = torch.zeros((DISTINCT, cap, 24), dtype=torch.uint8, device=dev)
            d = torch.zeros((DISTINCT, cap, 32), dtype=torch.uint8, device=dev)
            c = torch.zeros((DISTINCT,), dtype=torch.int32, device=dev)
        stream.synchronize()
        ext.extract_batch_device(img, DISTINCT, W, H, k, d, c, cap)
        ext.check()
        side.append((k, d, c))
    ext.close()
    reps_of = (B + DISTINCT - 1) // DISTINCT
    with torch.cuda.stream(stream):
        tile = lambda t: t.repeat((reps_of,) + (1,) * (t.dim() - 1))[:B].contiguous()   # noqa: E731
        il, ir = tile(left), tile(right)
        (kl, dl, nl), (kr, dr, nr) = [tuple(tile(t) for t in s) for s in side]
        obs = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
        m = torch.zeros((B, cap, 12), dtype=torch.uint8, device=dev)
        nm = torch.zeros((B,), dtype=torch.int32, device=dev)
        # the scale call: pose p relates pair p (train) to pair p + 1 (query) through the matches i <-> i, R = I, t = x
        rec = np.zeros(B - 1, POSE_RESULT_DTYPE)
        rec["R"], rec["t"], rec["valid"] = np.eye(3).reshape(-1), [1.0, 0.0, 0.0], 1
        n_id = int(min(nl.min().item(), 600))
        ident = np.zeros((B - 1, cap), MATCH_DTYPE)
        ident["query_idx"][:, :n_id] = ident["train_idx"][:, :n_id] = np.arange(n_id)
        d_rec = torch.from_numpy(rec.view(np.uint8)).to(dev)
        d_ident = torch.from_numpy(ident.view(np.uint8).reshape(-1)).to(dev)
        d_nid = torch.full((B - 1,), n_id, dtype=torch.int32, device=dev)
        d_scale = torch.zeros(((B - 1) * 16,), dtype=torch.uint8, device=dev)
    stream.synchronize()
    st = A.HipStereoMatcher(stream=stream.cuda_stream)

    def run_match():
        st.match_batch_device(il, ir, W * H, W, H, W, kl, dl, nl, kr, dr, nr, cap, B, obs, m, nm)

    def run_scale():
        st.scale_batch_device(d_rec, None, d_ident, d_nid, cap, obs.data_ptr() + cap * 32, nl.data_ptr() + 4, obs, nl, cap, B - 1,
                              d_scale)

    def timed(fn):
        for _ in range(warmup):
            fn()
        st.check()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(reps):
            t0.record(stream)
            fn()
            t1.record(stream)
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        st.check()
        return float(np.median(times)), float(np.min(times)), float(np.max(times))

    ms, ms_min, ms_max = timed(run_match)
    sms, sms_min, _ = timed(run_scale)
    matched = float(nm.float().mean().item())
    res = dict(width=W, height=H, features=nf, pairs=B, kp_stride=cap, left_keypoints=float(nl.float().mean().item()),
               right_keypoints=float(nr.float().mean().item()), matched_per_pair=matched, match_ms_median=ms, match_ms_min=ms_min,
               match_ms_max=ms_max, match_us_per_pair=ms * 1e3 / B, scale_matches=n_id, scale_ms_median=sms, scale_ms_min=sms_min,
               scale_us_per_pose=sms * 1e3 / (B - 1))
    print("%dx%d / %d features, %d pairs: match %.3f ms (median of %d, min %.3f max %.3f) = %.3f us/pair, %.0f of %.0f left "
          "keypoints matched; scale over %d matches %.3f ms = %.3f us/pose"
          % (W, H, nf, B, ms, reps, ms_min, ms_max, res["match_us_per_pair"], matched, res["left_keypoints"], n_id, sms,
             res["scale_us_per_pose"]))
    print(json.dumps(res))
    st.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--shapes", default="640x480x2000,752x480x1000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    assert torch.cuda.is_available(), "stereo_rate.py measures on the GPU; there is no CPU fallback"
    for shape in a.shapes.split(","):
        W, H, nf = (int(v) for v in shape.split("x"))
        measure(A, torch, W, H, nf, a.pairs, a.reps, a.warmup)


if __name__ == "__main__":
    main()
