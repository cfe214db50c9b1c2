#!/usr/bin/env python3
"""Rate of the batched loop alignment stage (aria_sim3_estimate_batch_device): 4096 pairs x 600 correspondences (40 % outliers)
at 1024 hypotheses by default -- the shape of tools/pnp_rate.py -- timed with HIP events on the aligner's stream after warm-up
launches, median of 20. Also the join (aria_sim3_associate_batch_device) of the same 4096 pairs against a map that the batch
triangulation of 4096 two-view scenes x 600 matches leaves in HBM (about 2 M points): keyframe 1 of pair p is view 2 of map pair
p, keyframe 2 its view 1, every match has a landmark on both sides. Then, in the same session, tools/pnp_rate.py at the same
shape as the yardstick (--no-yardstick skips it). Prints one JSON line.

No target is fixed in advance: Sim(3) scores two projections where PnP scores one, with a far cheaper solver.

Usage: sim3_rate.py [--pairs 4096] [--corr 600] [--outliers 0.4] [--hypotheses 1024] [--reps 20] [--no-assoc] [--no-yardstick]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(torch, stream, fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--corr", type=int, default=600)
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-assoc", action="store_true")
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import pose_ref as P
    from aria_slam_amd import sim3_ref as N

    dev = torch.device("cuda", 0)
    n, B = a.corr, a.pairs
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    # 64 distinct synthetic scenes (2-20 units, 0.5 px noise, 1 % depth noise, scales 0.5 to 2), tiled over the batch
    poses = []
    for s in range(64):
        R = P.rot([0.1 * (s % 3), 1.0, 0.2], 12.0 * (s % 4) / 3.0)
        poses.append((R, np.array([0.8 * np.cos(s), 0.2 * np.sin(3 * s), 0.4 * np.sin(s)]), 2.0 ** ((s % 5 - 2) / 2.0)))
    scenes = [N.synth_sim3(1000 + s, n, R, sc * t, sc, a.outliers, 0.5, depth_noise=0.01)[0].view(np.uint8).reshape(n, 64)
              for s, (R, t, sc) in enumerate(poses)]
    dcorr = d(np.stack([scenes[p % 64] for p in range(B)]))
    dn = d(np.full(B, n, np.int32))
    out = torch.zeros(B * 136, dtype=torch.uint8, device=dev)
    mask = torch.zeros(B * n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    al = A.HipSim3Aligner(hypotheses=a.hypotheses, stream=stream.cuda_stream)

    def run():
        al.estimate_batch_device(dcorr, dn, B, n, out, mask)

    for _ in range(a.warmup):
        run()
    al.check()
    times = _time(torch, stream, run, a.reps)
    al.check()
    rec = np.frombuffer(out.cpu().numpy().tobytes(), A._lib.SIM3_RESULT_DTYPE)
    ms = float(np.median(times))
    res = dict(pairs=B, corr=n, outliers=a.outliers, hypotheses=a.hypotheses, valid=int(rec["valid"].sum()),
               mean_inliers=float(rec["n_inliers"].mean()), mean_iterations=float(rec["iterations"].mean()),
               refined=int(rec["refined"].sum()), ms_median=ms, ms_min=float(np.min(times)), ms_max=float(np.max(times)),
               us_per_pair=ms * 1e3 / B, evals_per_s=float(B) * a.hypotheses * n / (ms * 1e-3))
    print("%d pairs x %d correspondences, %d hypotheses: %.3f ms (median of %d), %.3f us/pair, %.3g two-sided tests/s"
          % (B, n, a.hypotheses, ms, a.reps, res["us_per_pair"], res["evals_per_s"]))

    if not a.no_assoc:
        two = []
        for s, (R, t, _sc) in enumerate(poses):
            tu = np.array([1.0, 0.1 * np.sin(s), 0.0])
            tu = tu / np.linalg.norm(tu)
            kq, kt, m, _ = P.synth_two_view(2000 + s, n, R, tu, 0.0)
            ext = np.concatenate([np.hstack([np.eye(3), np.zeros((3, 1))]).ravel(), np.hstack([R, tu[:, None]]).ravel()])
            two.append((kq.view(np.uint8).reshape(n, 24), kt.view(np.uint8).reshape(n, 24), m.view(np.uint8).reshape(n, 12), ext))
        dkq, dkt, dmm = (d(np.stack([two[p % 64][k] for p in range(B)])) for k in range(3))
        dext = d(np.stack([two[p % 64][3] for p in range(B)]))
        danchor = d(np.arange(B, dtype=np.int32))
        dpose1 = d(np.stack([two[p % 64][3][12:] for p in range(B)]))       # keyframe 1 = view 2 of the map pair
        dpose2 = d(np.stack([two[p % 64][3][:12] for p in range(B)]))       # keyframe 2 = its view 1
        acorr = torch.zeros(B * n * 64, dtype=torch.uint8, device=dev)
        ancorr = torch.zeros(B, dtype=torch.int32, device=dev)
        aback = torch.zeros(B * n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        mp = A.HipMapper(capacity=B * n, stream=stream.cuda_stream)
        mp.triangulate_batch_device(dkq, dn, dkt, dn, n, dmm, dn, B, n, d_extrinsics=dext)
        mp.check()
        size = mp.size()

        def assoc():   # the matches pair keypoint i of view 1 with i of view 2: read as (query = view 2, train = view 1) they still do
            al.associate_batch_device(mp, danchor, danchor, 2, 1, dpose1, dpose2, dkt, dn, dkq, dn, n, dmm, dn, B, n, acorr, ancorr, aback)

        for _ in range(a.warmup):
            assoc()
        al.check()
        atimes = _time(torch, stream, assoc, a.reps)
        al.check()
        res.update(map_points=int(size), assoc_ms_median=float(np.median(atimes)), assoc_ms_min=float(np.min(atimes)),
                   assoc_ms_max=float(np.max(atimes)), assoc_corr=int(ancorr.sum().item()))
        print("join of %d pairs x %d matches against a map of %d points: %.3f ms (median of %d), %d correspondences"
              % (B, n, size, res["assoc_ms_median"], a.reps, res["assoc_corr"]))
        mp.close()
    al.close()
    if not a.no_yardstick:
        # a fresh process (this one has the GPU open; its program is not replaced), after this one's handles are closed
        cmd = [sys.executable, os.path.join(ROOT, "tools", "pnp_rate.py"), "--pairs", str(B), "--corr", str(n), "--outliers",
               str(a.outliers), "--hypotheses", str(a.hypotheses), "--reps", str(a.reps)]
        y = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if y.returncode != 0:
            raise SystemExit("pnp_rate.py failed:\n" + y.stdout + y.stderr)
        pnp = json.loads(y.stdout.strip().splitlines()[-1])
        res["pnp"] = {k: pnp[k] for k in ("ms_median", "us_per_pair", "evals_per_s", "assoc_ms_median", "map_points") if k in pnp}
        res["ratio_to_pnp"] = res["ms_median"] / pnp["ms_median"]
        if "assoc_ms_median" in res and "assoc_ms_median" in pnp:
            res["assoc_ratio_to_pnp"] = res["assoc_ms_median"] / pnp["assoc_ms_median"]
        print("yardstick: PnP (DLT) at the same shape %.3f ms: Sim(3) takes %.2f of it" % (pnp["ms_median"], res["ratio_to_pnp"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
