#!/usr/bin/env python3
"""Rate of the visual-inertial fusion stage (aria_fuse_run_batch_device, aria_fuse_preintegrate_batch_device), timed with HIP
events on the handle's stream (median of 20; the filter records are restored on the same stream before every call, outside
the timed interval):
  long    one track of 36 000 samples and 3 600 frames (180 s of the scene of aria_slam_amd.fusion_ref.make_scene)
  wide    4096 tracks x 4 000 samples x 400 frames: one 20 s scene under 4096 noise settings (the six constants of each filter
          record spread over a decade), which is the sweep a user of this stage does first
  ragged  the same with the tracks cut to lengths spread 4:1
  preint  100 000 intervals of 10 samples
An event is one IMU sample or one accepted visual record. Prints ms per call, ns per event (per track: ms / events of all
tracks), the tracks in flight, and the NumPy restatement's time per event on the host -- a Python loop, NOT Eigen: the
ratio says how far a batch on the device is from the definition's own speed, not from the reference's. One JSON line per case.

Usage: fuse_rate.py [--tracks 4096] [--reps 20] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, stream, reps, warmup, restore, call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(warmup + reps):
        with torch.cuda.stream(stream):
            restore()
        t0.record(stream)
        call()
        t1.record(stream)
        t1.synchronize()
        if k >= warmup:
            times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(np.min(times))


def run_case(A, torch, name, imu, ends, viss, filters, reps, warmup):
    """imu: one (N, 7) array shared by every track (track k uses its first ends[k][-1] samples)."""
    from aria_slam_amd import _lib
    from aria_slam_amd import fusion as FU
    dev = torch.device("cuda", 0)
    B = len(ends)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    rec = FU.pack_imu(imu)
    n_s = [int(e[-1]) for e in ends]
    ioff = np.concatenate([[0], np.cumsum(n_s)]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([len(e) for e in ends])]).astype(np.int64)
    assert ioff[-1] < 2 ** 31 and foff[-1] < 2 ** 31
    d_one = d(rec)
    d_imu = torch.cat([d_one[:n * _lib.IMU_SAMPLE_DTYPE.itemsize] for n in n_s] + [d_one[:56]])
    d_end = d(np.concatenate(list(ends) + [np.zeros(1, np.int32)]).astype(np.int32))
    d_vis = d(np.concatenate([FU.pack_visual(v) for v in viss] + [np.zeros(1, _lib.FUSE_VISUAL_DTYPE)]))
    d_io, d_fo = d(ioff.astype(np.int32)), d(foff.astype(np.int32))
    pristine = d(filters)
    d_flt = pristine.clone()
    d_st = torch.zeros((int(foff[-1]) + 1) * _lib.FUSE_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    fu = A.HipSensorFusion(stream=stream.cuda_stream)
    ms, ms_min = timed(torch, stream, reps, warmup, lambda: d_flt.copy_(pristine),
                       lambda: fu.run_batch_device(d_flt, d_imu, d_io, int(ioff[-1]), d_end, d_vis, d_fo, int(foff[-1]), B, d_st))
    fu.check()
    st = np.frombuffer(d_st.cpu().numpy().tobytes(), _lib.FUSE_STATE_DTYPE)[:int(foff[-1])]
    fu.close()
    events = int(st["n_predicted"].sum() + st["n_skipped"].sum() + st["n_updates"].sum())
    out = dict(case=name, tracks=B, samples=int(ioff[-1]), frames=int(foff[-1]), events=events, ms_median=ms, ms_min=ms_min,
               ns_per_event_per_track=ms * 1e6 / max(events, 1), us_per_event_of_the_longest_track=ms * 1e3 / (max(n_s) + max(len(e) for e in ends)),
               tracks_in_flight=B, valid=int(st["valid"].sum()), finite=bool(np.isfinite(st["p"]).all()))
    print("%s: %d track%s, %d samples, %d frames: %.3f ms per call (median of %d, min %.3f), %.1f ns per event per track, %.2f us "
          "per step of the longest track, %d tracks in flight" % (name, B, "" if B == 1 else "s", out["samples"], out["frames"], ms,
                                                                  reps, ms_min, out["ns_per_event_per_track"],
                                                                  out["us_per_event_of_the_longest_track"], B))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--intervals", type=int, default=100000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    from aria_slam_amd import fusion_ref as R
    from aria_slam_amd import fusion as FU
    from aria_slam_amd import _lib

    long_sc = R.make_scene(21, duration=180.0)
    sc = R.make_scene(22, duration=20.0)
    host_us = None
    if not a.no_host:
        t = time.perf_counter()
        R.run_track(R.SensorFusion(), sc["imu"][:2000], sc["imu_end"][:201], sc["visual"][:201])
        host_us = (time.perf_counter() - t) * 1e6 / 2200
        t = time.perf_counter()
        R.preintegrate(sc["imu"], np.arange(0, 2000, 10), np.arange(10, 2010, 10))
        host_pre_us = (time.perf_counter() - t) * 1e6 / 200
        print("host: the NumPy restatement takes %.1f us per event, %.1f us per 10-sample interval (a Python loop, not Eigen)" %
              (host_us, host_pre_us))

    import torch
    import aria_slam_amd as A
    B = a.tracks
    rng = np.random.default_rng(0)
    filters = FU.new_filter(B)
    for k in ("accel_noise", "gyro_noise", "accel_bias_walk", "gyro_bias_walk", "pos_noise", "rot_noise"):
        filters[k] = filters[k] * 10.0 ** rng.uniform(-0.5, 0.5, B)
    results = []
    results.append(run_case(A, torch, "long", long_sc["imu"], [long_sc["imu_end"][:3600]], [long_sc["visual"][:3600]],
                            FU.new_filter(1), a.reps, a.warmup))
    end400, vis400 = sc["imu_end"][:400], FU.pack_visual(sc["visual"][:400])
    # frame 0 has no samples before it: 400 frames consume 3990 samples; the 401st frame's 10 complete the 4000
    end400 = end400.copy()
    end400[-1] = 4000
    results.append(run_case(A, torch, "wide", sc["imu"], [end400] * B, [vis400] * B, filters, a.reps, a.warmup))
    lens = np.linspace(100, 400, B).astype(int)
    rng.shuffle(lens)
    results.append(run_case(A, torch, "ragged", sc["imu"], [sc["imu_end"][:n] for n in lens], [vis400[:n] for n in lens], filters,
                            a.reps, a.warmup))
    # preintegration
    dev = torch.device("cuda", 0)
    N = a.intervals
    imu = np.tile(sc["imu"], (N * 10 // len(sc["imu"]) + 1, 1))[:N * 10].copy()
    imu[:, 0] = sc["imu"][0, 0] + 0.005 * np.arange(len(imu))
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    d_imu, d_b, d_e = d(FU.pack_imu(imu)), d(np.arange(0, N * 10, 10, dtype=np.int32)), d(np.arange(10, N * 10 + 10, 10, dtype=np.int32))
    d_out = torch.zeros(N * _lib.PREINT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    pre = A.HipImuPreintegrator(stream=stream.cuda_stream)
    ms, ms_min = timed(torch, stream, a.reps, a.warmup, lambda: None,
                       lambda: pre.preintegrate_device(d_imu, len(imu), d_b, d_e, N, None, d_out))
    pre.check()
    res = np.frombuffer(d_out.cpu().numpy().tobytes(), _lib.PREINT_RESULT_DTYPE)
    pre.close()
    out = dict(case="preint", intervals=N, samples=len(imu), ms_median=ms, ms_min=ms_min, ns_per_interval=ms * 1e6 / N,
               valid=int(res["valid"].sum()), used=int(res["n_used"].sum()))
    print("preint: %d intervals of 10 samples: %.3f ms per call (median of %d, min %.3f), %.1f ns per interval" %
          (N, ms, a.reps, ms_min, out["ns_per_interval"]))
    results.append(out)
    for r in results:
        if host_us is not None:
            r["host_numpy_us_per_event"] = host_us
        print(json.dumps(r))


if __name__ == "__main__":
    main()
