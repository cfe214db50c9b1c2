#!/usr/bin/env python3
"""Rate of the obstacle-alert stage (aria_alert_measure_batch_device, aria_alert_arbitrate_batch_device) at 752 x 480 with the
default band, inputs resident in HBM, timed with HIP events on the handle's stream: 3 warm-up calls, then the median of 20.

Measured, each step in a process of its own under its own time limit (a step that fails or runs out of time ends the tool:
nothing more is started on the GPU):
  measure    rules 1-2 over 256 seeded depth maps (370 MB, more than the Infinity Cache holds) with 16 seeded boxes a frame:
             us per frame and the share of 8 TB/s that aria_alert_algorithmic_bytes over that time comes to;
  arbitrate  rules 3-6 over 256 tracks of 256 frames each (65 536 frames of random measurements and 16 boxes a frame).
With --select-ab (needs the variants build, which knows ARIA_ALERT_SELECT) a second handle measures with the plainest exact
selection, a 32-pass bitwise bisection that re-reads the rectangle every pass, alternating with the shipped kernel inside one
run, so that the gain of the radix selection is a measured ratio. Both handles' records are compared bitwise, and two frames
against the restatement. There is no pass or fail on time. Prints a table and writes one JSON line per measurement to --out.

Usage: alert_rate.py [--frames 256] [--boxes 16] [--tracks 256] [--reps 20] [--warmup 3] [--select-ab] [--out profiles/alert_rate.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_SECONDS = {"measure": 240, "arbitrate": 240}
PEAK_BYTES_PER_S = 8e12


def seeded_frames(n, boxes, W=752, H=480):
    """(depth [n, H, W], dets [n, boxes], ndets [n]): a ground ramp with speckle and holes, and boxes of 20..300 px."""
    from aria_slam_amd.alert_ref import DETECTION_DTYPE
    rng = np.random.default_rng(2024)
    yy = np.arange(H, dtype=np.float32)[:, None]
    ramp = (np.float32(0.6) + (np.float32(H) - yy) * np.float32(0.03)).astype(np.float32)
    depth = np.empty((n, H, W), np.float32)
    for f in range(n):
        d = ramp + rng.random((H, W), dtype=np.float32) * np.float32(1.5)
        d[rng.random((H, W), dtype=np.float32) < 0.12] = 0.0
        depth[f] = d
    dets = np.zeros((n, boxes), DETECTION_DTYPE)
    x1 = rng.integers(0, W - 20, (n, boxes)).astype(np.float32)
    y1 = rng.integers(0, H - 20, (n, boxes)).astype(np.float32)
    dets["x1"], dets["y1"] = x1, y1
    dets["x2"] = x1 + rng.integers(20, 300, (n, boxes)).astype(np.float32)
    dets["y2"] = y1 + rng.integers(20, 300, (n, boxes)).astype(np.float32)
    dets["confidence"] = 0.9
    dets["class_id"] = rng.integers(0, 80, (n, boxes))
    return depth, dets, np.full(n, boxes, np.int32)


def timed(torch, stream, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def step_measure(a):
    if a.select_ab:
        os.environ["ARIA_ORB_HIP_LIBRARY"] = os.path.join(ROOT, "aria_slam_amd", "libaria_orb_hip_variants.so")
        assert os.path.exists(os.environ["ARIA_ORB_HIP_LIBRARY"]), "--select-ab needs `make -C aria_slam_amd/csrc variants`"
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import alert, alert_ref as R
    assert torch.cuda.is_available(), "alert_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    cfg = R.config()
    n, W, H = a.frames, cfg.width, cfg.height
    depth, dets, ndets = seeded_frames(n, a.boxes)
    with torch.cuda.stream(stream):
        d_depth = torch.from_numpy(depth).to(dev)
        d_dets = torch.from_numpy(dets.view(np.uint8).reshape(-1)).to(dev)
        d_ndets = torch.from_numpy(ndets).to(dev)
        d_meas = {name: torch.zeros(n * 64 * 16, dtype=torch.uint8, device=dev) for name in ("radix", "plain")}
    stream.synchronize()
    handles = {"radix": A.HipObstacleAlerter(stream=stream.cuda_stream)}
    if a.select_ab:
        os.environ["ARIA_ALERT_SELECT"] = "plain"
        handles["plain"] = A.HipObstacleAlerter(stream=stream.cuda_stream)
        del os.environ["ARIA_ALERT_SELECT"]
    times = {name: [] for name in handles}
    for rep in range(a.warmup + a.reps):
        for name, h in handles.items():                              # alternating: both selections see the same clocks and caches
            ms = timed(torch, stream, lambda: h.measure_batch_device(d_depth, W * H, W, n, d_meas[name], d_dets, d_ndets, a.boxes))
            if rep >= a.warmup:
                times[name].append(ms)
    algo = alert.algorithmic_bytes(W, cfg.zone_top, cfg.zone_bottom, n)
    results, got = [], {}
    for name, h in handles.items():
        assert h.status() == 0
        got[name] = d_meas[name].cpu().numpy().view(R.MEAS_DTYPE).reshape(n, 64)
        t = times[name]
        med = float(np.median(t))
        res = dict(stage="measure", select=name, size=[W, H], band=[cfg.zone_top, cfg.zone_bottom], frames=n, boxes=a.boxes, ms_median=med,
                   ms_min=float(np.min(t)), ms_max=float(np.max(t)), us_per_frame=med * 1e3 / n, algorithmic_bytes=int(algo),
                   share_of_8TBps=algo / (med * 1e-3) / PEAK_BYTES_PER_S)
        results.append(res)
        print("%-6s measure %9.3f ms (min %.3f max %.3f) %.2f us/frame, %.1f %% of 8 TB/s on the algorithmic bytes"
              % (name, med, res["ms_min"], res["ms_max"], res["us_per_frame"], 100 * res["share_of_8TBps"]))
        h.close()
    want = R.measure(depth[:2], cfg, dets[:2], ndets[:2])[0]
    assert got["radix"][:2].tobytes() == want.tobytes(), "the shipped selection differs from the restatement"
    if a.select_ab:
        assert got["radix"].tobytes() == got["plain"].tobytes(), "the selections disagree"
        r = {x["select"]: x for x in results}
        print("measure, 32-pass bisection vs shipped radix selection: %.2fx" % (r["plain"]["ms_median"] / r["radix"]["ms_median"]))
        results.append(dict(stage="measure", select="plain/radix", ratio=r["plain"]["ms_median"] / r["radix"]["ms_median"], bitwise_equal=True))
    return results


def step_arbitrate(a):
    import torch
    import aria_slam_amd as A
    from aria_slam_amd import alert_ref as R
    assert torch.cuda.is_available(), "alert_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    cfg = R.config()
    T, per, B = a.tracks, 256, a.boxes
    n = T * per
    rng = np.random.default_rng(77)
    dist = np.array([0.4, 0.9, 1.0, 1.2, 1.5, 1.9, 2.0, 2.4, 3.0, 3.5, 6.0], np.float32)
    meas = np.zeros((n, 64), R.MEAS_DTYPE)
    meas["distance"] = np.float32(-1.0)
    used = 3 + B
    has = rng.random((n, used)) < 0.7
    meas["flags"][:, :used] = np.where(has, R.MEAS_SOURCE | R.MEAS_OK, R.MEAS_SOURCE)
    meas["distance"][:, :used] = np.where(has, dist[rng.integers(0, len(dist), (n, used))], np.float32(-1.0))
    meas["n_valid"][:, :used] = np.where(has, 100, 0)
    meas["k"][:, :used] = np.where(has, 50, 0)
    _, dets, ndets = seeded_frames(1, B)
    dets = np.repeat(dets, n, axis=0)
    dets["class_id"] = rng.integers(0, 80, (n, B))
    dets["x1"] = rng.integers(0, 700, (n, B)).astype(np.float32)
    dets["x2"] = dets["x1"] + 50
    ndets = np.full(n, B, np.int32)
    ts = (1403636579763555584 + np.tile(np.arange(per, dtype=np.int64) * 50_000_000, T)).astype(np.int64)
    off = (np.arange(T + 1) * per).astype(np.int32)
    cap = 2 * per
    with torch.cuda.stream(stream):
        d = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to(dev)
             for k, v in dict(meas=meas, dets=dets, ndets=ndets, ts=ts, off=off).items()}
        d_states = torch.zeros(T * 2320, dtype=torch.uint8, device=dev)
        d_events = torch.zeros(T * cap * 32, dtype=torch.uint8, device=dev)
        d_nev = torch.zeros(T, dtype=torch.int32, device=dev)
    stream.synchronize()
    h = A.HipObstacleAlerter(stream=stream.cuda_stream)
    times = []
    for rep in range(a.warmup + a.reps):
        with torch.cuda.stream(stream):
            d_states.zero_()
        ms = timed(torch, stream, lambda: h.arbitrate_batch_device(d["off"], T, d["ts"], n, d["meas"], d_states, d_events, cap, d_nev,
                                                                   d["dets"], d["ndets"], B))
        if rep >= a.warmup:
            times.append(ms)
    assert h.status() == 0
    nev = d_nev.cpu().numpy()
    ev = d_events.cpu().numpy().view(R.EVENT_DTYPE).reshape(T, cap)
    states = R.new_state(2)
    want, want_n, _ = R.arbitrate(cfg, off[:3], ts, meas, states, cap, dets, ndets)
    for t in range(2):
        assert nev[t] == want_n[t] and ev[t, :nev[t]].tobytes() == want[t].tobytes(), "track %d differs from the restatement" % t
    h.close()
    med = float(np.median(times))
    res = dict(stage="arbitrate", tracks=T, frames_per_track=per, boxes=B, ms_median=med, ms_min=float(np.min(times)), ms_max=float(np.max(times)),
               us_per_frame=med * 1e3 / n, events=int(nev.sum()))
    print("arbitrate %9.3f ms (min %.3f max %.3f) %d tracks x %d frames, %.3f us per frame, %d events"
          % (med, res["ms_min"], res["ms_max"], T, per, res["us_per_frame"], res["events"]))
    return [res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--select-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alert_rate.json"))
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), help="run one step in this process and print its JSON lines (what the tool starts)")
    a = ap.parse_args()
    if a.step:
        for r in {"measure": step_measure, "arbitrate": step_arbitrate}[a.step](a):
            print("JSON " + json.dumps(r))
        return 0
    lines = []
    for step in ("measure", "arbitrate"):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--frames", str(a.frames),
               "--boxes", str(a.boxes), "--tracks", str(a.tracks), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        if a.select_ab:
            cmd.append("--select-ab")
        p = subprocess.run(cmd, capture_output=True, text=True)
        for l in p.stdout.splitlines():
            if l.startswith("JSON "):
                lines.append(l[5:])
            else:
                print(l)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            print("step %s ended with status %d: nothing more is started" % (step, p.returncode))
            return p.returncode
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for l in lines:
            f.write(l + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
