"""Visual-inertial fusion on the MI355X (aria_fuse_*, kernels in aria_slam_amd/csrc/imu_fusion.hip) against the NumPy
restatement (aria_slam_amd/fusion_ref.py): every per-frame state, the final filter record with the whole of P, the counters;
preintegration; aria_fuse_visual_from_pose_device and the device-resident chain; bitwise determinism over runs, batch
position, batch split, chunked feeding, wave neighbours and per-track noise constants; invalid tracks and the edges of the
input space; the Python class.

Tolerance: measured, not chosen. The yardstick is fusion_ref run in np.longdouble. For each track below, GAP is the largest
absolute difference between the restatement's fp64 run and its extended run, measured on the CPU (states: metres, m/s,
quaternion and bias entries; P and the preintegration covariance: relative to their largest entry). The device is allowed
10 * GAP against the extended run: one decade for a different summation order in the covariance products and another
sin / cos / atan2. Nothing is compared against the device's own output except where bits must be identical.

GAP as measured (tools/fuse_gap.py prints this table):
    track      states     P (rel)
    scene1     4.88e-15   7.40e-15
    scene2     4.53e-15   7.40e-15
    scene3     5.04e-15   7.41e-15
    dropout    1.13e-14   2.34e-14
    imugap     3.62e-15   9.99e-15
    repeat     3.49e-15   8.93e-15
    relpose    1.68e-14   2.36e-14
    long300    6.07e-15   2.16e-14
    preint     1.68e-15   2.07e-15
What the device showed against the extended run is printed by the tests and recorded in DESIGN.md section 14."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")

ARIA_E_INVALID = -1
# measured on the CPU with the committed restatement (tools/fuse_gap.py); (states, P relative)
GAP = {
    "scene1": (4.88e-15, 7.40e-15),
    "scene2": (4.53e-15, 7.40e-15),
    "scene3": (5.04e-15, 7.41e-15),
    "dropout": (1.13e-14, 2.34e-14),
    "imugap": (3.62e-15, 9.99e-15),
    "repeat": (3.49e-15, 8.93e-15),
    "relpose": (1.68e-14, 2.36e-14),
    "long300": (6.07e-15, 2.16e-14),
}
GAP_PREINT = (1.68e-15, 2.07e-15)     # (delta_p / delta_v / delta_q / dt_sum, covariance relative) over PREINT intervals
STATE_KEYS = ("p", "v", "q", "ba", "bg")
COUNTERS = ("n_predicted", "n_skipped", "n_ignored", "n_updates", "initialized")
TRACKS = ["scene1", "scene2", "scene3", "dropout", "imugap", "repeat", "relpose", "long300"]


def make_track(name):
    """(imu (N, 7), imu_end (F,), visual [(t, R, p, accept)]) of a named test track; CPU only."""
    from aria_slam_amd import fusion_ref as R
    if name.startswith("scene"):
        sc = R.make_scene(int(name[5:]))
        return sc["imu"], sc["imu_end"], sc["visual"]
    if name == "long300":
        sc = R.make_scene(7, duration=300.0)
        return sc["imu"], sc["imu_end"], sc["visual"]
    sc = R.make_scene(11, duration=10.0)
    imu, end, vis = sc["imu"].copy(), sc["imu_end"].copy(), list(sc["visual"])
    if name == "dropout":          # no accepted pose for 2 s
        vis = [(t, Rm, p, 0 if 40 <= f < 80 else 1) for f, (t, Rm, p, _a) in enumerate(vis)]
    elif name == "imugap":         # 0.15 s of samples missing: the next sample only moves the time
        keep = np.ones(len(imu), bool)
        keep[600:630] = False
        end = np.array([int(keep[:e].sum()) for e in end], np.int32)
        imu = imu[keep]
    elif name == "repeat":         # a timestamp twice (dt = 0) and one going backwards (dt < 0)
        imu[500, 0] = imu[499, 0]
        imu[900, 0] = imu[898, 0]
    else:
        assert name == "relpose"   # what src/euroc_eval.cpp:209 feeds: the relative R, t of recoverPose, |t| = 1
        truth_p, truth_R = sc["truth_p"], sc["truth_R"]
        rel = [(vis[0][0], np.eye(3), np.array([0.0, 0.0, 1.0]), 1)]
        for f in range(1, len(vis)):
            Rr = truth_R[f].T @ truth_R[f - 1]
            tr = truth_R[f].T @ (truth_p[f - 1] - truth_p[f])
            rel.append((vis[f][0], Rr, tr / np.linalg.norm(tr), 0 if f % 7 == 3 else 1))
        vis = rel
    return imu, end, vis


_ref_cache = {}


def ref_runs(name):
    """(fp64 states, fp64 filter, extended states, extended filter) of the restatement on a track."""
    from aria_slam_amd import fusion_ref as R
    if name not in _ref_cache:
        imu, end, vis = make_track(name)
        f64, fld = R.SensorFusion(), R.SensorFusion(np.longdouble)
        _ref_cache[name] = (R.run_track(f64, imu, end, vis), f64, R.run_track(fld, imu, end, vis), fld)
    return _ref_cache[name]


PREINT_N = 3000


def make_intervals():
    """(imu, begin, end, bias): PREINT_N intervals over a scene's samples, with empty, one-sample and gap intervals."""
    from aria_slam_amd import fusion_ref as R
    imu = R.make_scene(5, duration=30.0)["imu"].copy()
    imu[1000:, 0] += 0.6           # a gap over 0.5 s
    imu[2000, 0] = imu[1999, 0]    # dt = 0
    imu[3000:, 0] += 0.3           # a gap under 0.5 s: integrated
    rng = np.random.default_rng(3)
    begin = rng.integers(0, len(imu) - 40, PREINT_N).astype(np.int32)
    length = rng.integers(0, 40, PREINT_N)
    length[:50] = 0
    length[50:100] = 1
    begin[100:110] = np.arange(990, 1000)
    length[100:110] = 20
    begin[110:120] = np.arange(1990, 2000)
    length[110:120] = 20
    begin[120:130] = np.arange(2990, 3000)
    length[120:130] = 20
    return imu, begin, (begin + length).astype(np.int32), np.array([0.05, -0.03, 0.02, 0.002, -0.001, 0.0015])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fu(aria):
    o = aria.HipSensorFusion()
    yield o
    o.close()


def _state_diff(st, ref):
    return max(float(np.abs(st[k].astype(np.longdouble) - ref[k]).max()) for k in STATE_KEYS)


@pytest.mark.parametrize("name", TRACKS)
def test_device_matches_the_restatement(aria, fu, name):
    from aria_slam_amd import fusion as FU
    imu, end, vis = make_track(name)
    _s64, _f64, sld, fld = ref_runs(name)
    gap_s, gap_p = GAP[name]
    filt = FU.new_filter(1)
    st = fu.run(imu, end, vis, filt)
    assert st["valid"].all() and np.isfinite(st["p"]).all() and np.isfinite(filt[0]["P"]).all()
    for k in COUNTERS:
        assert np.array_equal(st[k], sld[k]), k
    assert np.array_equal(st["t"], np.array([v[0] for v in vis]))
    ds = _state_diff(st, sld)
    pmax = float(np.abs(fld.P).max())
    dd = float(np.abs(st["P_diag"].astype(np.longdouble) - sld["P_diag"]).max() / max(float(np.abs(sld["P_diag"]).max()), 1e-300))
    dp = float(np.abs(filt[0]["P"].reshape(15, 15).astype(np.longdouble) - fld.P).max() / pmax)
    fin = FU.filter_from_ref(fld)[0]
    dfin = max(float(np.abs(filt[0][k] - fin[k]).max()) for k in STATE_KEYS)
    print("%s: states %.2e (allowed %.2e)  P_diag rel %.2e  final P rel %.2e (allowed %.2e)  final state %.2e" %
          (name, ds, 10 * gap_s, dd, dp, 10 * gap_p, dfin))
    assert ds <= 10 * gap_s and dfin <= 10 * gap_s
    assert dd <= 10 * gap_p and dp <= 10 * gap_p
    assert filt[0]["last_imu_time"] == float(fld.last_imu_time) and filt[0]["last_visual_time"] == float(fld.last_visual_time)
    assert filt[0]["initialized"] == 1
    P = filt[0]["P"].reshape(15, 15)
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P).min() > 0


def test_preintegration_matches_the_restatement(aria):
    from aria_slam_amd import fusion_ref as R
    imu, begin, end, bias = make_intervals()
    pre = aria.HipImuPreintegrator()
    out = pre.preintegrate(imu, begin, end, bias)
    ref = R.preintegrate(imu, begin, end, bias, dtype=np.longdouble)
    assert out["valid"].all() and np.array_equal(out["n_used"], ref["n_used"])
    assert (out["n_used"][:100] == 0).all() and not out["cov"][:100].any() and (out["delta_q"][:100, 0] == 1).all()
    ds = max(float(np.abs(out[k].astype(np.longdouble) - ref[k]).max()) for k in ("delta_p", "delta_v", "delta_q", "dt_sum"))
    cmax = float(np.abs(ref["cov"]).max())
    dc = float(np.abs(out["cov"].reshape(-1, 9, 9).astype(np.longdouble) - ref["cov"]).max()) / cmax
    print("preintegration: deltas %.2e (allowed %.2e)  covariance rel %.2e (allowed %.2e)" %
          (ds, 10 * GAP_PREINT[0], dc, 10 * GAP_PREINT[1]))
    assert ds <= 10 * GAP_PREINT[0] and dc <= 10 * GAP_PREINT[1]
    # without a bias, and bitwise again; an invalid interval is zeroed and flagged, its neighbours untouched
    again = pre.preintegrate(imu, begin, end, bias)
    assert again.tobytes() == out.tobytes()
    b2, e2 = begin.copy(), end.copy()
    b2[7], e2[7] = 50, 40
    e2[9] = len(imu) + 1
    b2[11] = -1
    bad = imu.copy()
    bad[int(begin[200]), 2] = np.nan
    got = pre.preintegrate(bad, b2, e2, bias, raise_on_error=False)
    assert pre.last_status == ARIA_E_INVALID
    hit = np.array([(b2[i] <= begin[200] < e2[i]) for i in range(len(b2))]) | np.isin(np.arange(len(b2)), [7, 9, 11])
    assert hit[200] or end[200] == begin[200]
    assert not got["valid"][hit].any() and not got[hit].tobytes().strip(b"\0")
    assert got[~hit].tobytes() == out[~hit].tobytes()
    assert pre.status() == 0
    pre.close()


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda")


def _launch(torch, fu, filters, tracks, ioff=None, foff=None, vis_dev=None):
    """Raw aria_fuse_run_batch_device over concatenated tracks; offsets can be overridden. Returns (filters, states, status,
    frame offsets)."""
    from aria_slam_amd import _lib
    from aria_slam_amd import fusion as FU
    imus = [FU.pack_imu(t[0]) for t in tracks]
    ends = [np.asarray(t[1], np.int32).reshape(-1) for t in tracks]
    viss = [FU.pack_visual(t[2]) for t in tracks]
    io = np.concatenate([[0], np.cumsum([len(x) for x in imus])]).astype(np.int32) if ioff is None else np.asarray(ioff, np.int32)
    fo = np.concatenate([[0], np.cumsum([len(x) for x in viss])]).astype(np.int32) if foff is None else np.asarray(foff, np.int32)
    allimu = np.concatenate(imus + [np.zeros(1, _lib.IMU_SAMPLE_DTYPE)])
    allend = np.concatenate(ends + [np.zeros(1, np.int32)])
    allvis = np.concatenate(viss + [np.zeros(1, _lib.FUSE_VISUAL_DTYPE)])
    n_imu, n_fr = len(allimu) - 1, len(allvis) - 1
    dflt, dimu, dio, dend, dfo = _dev(torch, filters), _dev(torch, allimu), _dev(torch, io), _dev(torch, allend), _dev(torch, fo)
    dvis = _dev(torch, allvis) if vis_dev is None else vis_dev
    dst = torch.full(((n_fr + 1) * _lib.FUSE_STATE_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fu.run_batch_device(dflt, dimu, dio, n_imu, dend, dvis, dfo, n_fr, len(tracks), dst)
    status = fu.status()
    f = np.frombuffer(dflt.cpu().numpy().tobytes(), _lib.FUSE_FILTER_DTYPE).copy()
    s = np.frombuffer(dst.cpu().numpy().tobytes(), _lib.FUSE_STATE_DTYPE)[:n_fr].copy()
    return f, s, status, fo


def _short(name, frames):
    imu, end, vis = make_track(name)
    return imu[:int(end[frames - 1])], end[:frames], vis[:frames]


def test_bitwise_runs_position_split_chunks_neighbours_and_noise(aria, fu, torch_cuda):
    from aria_slam_amd import fusion as FU
    from aria_slam_amd import fusion_ref as R
    torch = torch_cuda
    # tracks of different length in one launch: 9 tracks over three waves, lengths spread 8:1
    names = ["scene1", "dropout", "imugap", "repeat", "relpose", "scene2", "scene3", "scene1", "dropout"]
    frames = [400, 50, 190, 120, 77, 401, 64, 100, 180]
    tracks = [_short(n, f) for n, f in zip(names, frames)]
    filt = FU.new_filter(len(tracks))
    filt["accel_noise"][5], filt["pos_noise"][5], filt["gravity"][5] = 0.3, 0.02, (0.0, 0.0, -9.80)      # per-track constants
    f1, s1, st, fo = _launch(torch, fu, filt, tracks)
    assert st == 0 and s1["valid"].all()
    # second run
    f2, s2, st, _ = _launch(torch, fu, filt, tracks)
    assert f1.tobytes() == f2.tobytes() and s1.tobytes() == s2.tobytes()
    # every track alone (host form, another place in another wave): a track's bits do not depend on its neighbours
    for k, tr in enumerate(tracks):
        one = filt[k:k + 1].copy()
        so = fu.run(tr[0], tr[1], tr[2], one)
        assert one.tobytes() == f1[k:k + 1].tobytes(), k
        assert so.tobytes() == s1[fo[k]:fo[k + 1]].tobytes(), k
    # batch position and batch split
    order = [4, 8, 0, 6, 2, 5, 1, 7, 3]
    f3, s3, st, fo3 = _launch(torch, fu, filt[order], [tracks[k] for k in order])
    for pos, k in enumerate(order):
        assert f3[pos:pos + 1].tobytes() == f1[k:k + 1].tobytes()
        assert s3[fo3[pos]:fo3[pos + 1]].tobytes() == s1[fo[k]:fo[k + 1]].tobytes()
    fa, sa, st, _ = _launch(torch, fu, filt[:4], tracks[:4])
    fb, sb, st, _ = _launch(torch, fu, filt[4:], tracks[4:])
    assert fa.tobytes() + fb.tobytes() == f1.tobytes() and sa.tobytes() + sb.tobytes() == s1.tobytes()
    # chunked feeding through the filter record
    imu, end, vis = tracks[0]
    one = filt[0:1].copy()
    got = []
    cuts = [0, 1, 2, 19, 150, len(vis)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s0 = int(end[lo - 1]) if lo else 0
        got.append(fu.run(imu[s0:int(end[hi - 1])], end[lo:hi] - s0, vis[lo:hi], one))
    assert one.tobytes() == f1[0:1].tobytes() and np.concatenate(got).tobytes() == s1[fo[0]:fo[1]].tobytes()
    # the track with its own constants follows the restatement run with them, and differs from the default one
    ref = R.SensorFusion(np.longdouble, gravity=(0.0, 0.0, -9.80), accel_noise=0.3, pos_noise=0.02)
    want = R.run_track(ref, *tracks[5])
    ds = _state_diff(s1[fo[5]:fo[6]], want)
    dp = float(np.abs(f1[5]["P"].reshape(15, 15).astype(np.longdouble) - ref.P).max() / np.abs(ref.P).max())
    print("per-track constants: states %.2e  P rel %.2e" % (ds, dp))
    assert ds <= 10 * GAP["scene2"][0] and dp <= 10 * GAP["scene2"][1]
    dflt = fu.run(*tracks[5], FU.new_filter(1))
    assert np.abs(dflt["p"] - s1[fo[5]:fo[6]]["p"]).max() > 1e-6


def test_invalid_tracks_are_flagged_untouched_and_do_not_disturb_neighbours(aria, fu, torch_cuda):
    from aria_slam_amd import fusion as FU
    torch = torch_cuda
    good = [_short("scene1", 60), _short("dropout", 90), _short("scene2", 30)]
    fg, sg, st, fog = _launch(torch, fu, FU.new_filter(3), good)
    assert st == 0

    def variant(kind):
        imu, end, vis = _short("scene3", 40)
        imu, end, vis = imu.copy(), end.copy(), list(vis)
        if kind == "nan sample":
            imu[123, 5] = np.nan
        elif kind == "inf time":
            imu[7, 0] = np.inf
        elif kind == "nan measurement":
            vis[12] = (vis[12][0], vis[12][1], np.array([0.0, np.nan, 0.0]), 1)
        elif kind == "nan rotation of a rejected frame":
            Rm = vis[13][1].copy()
            Rm[1, 1] = np.nan
            vis[13] = (vis[13][0], Rm, vis[13][2], 0)
        elif kind == "inf visual time":
            vis[3] = (-np.inf, vis[3][1], vis[3][2], 1)
        elif kind == "imu_end decreasing":
            end[20] = end[19] - 1
        elif kind == "imu_end beyond the samples":
            end[-1] = len(imu) + 1
        else:
            assert kind == "imu_end negative"
            end[0] = -1
        return imu, end, vis

    kinds = ["nan sample", "inf time", "nan measurement", "nan rotation of a rejected frame", "inf visual time",
             "imu_end decreasing", "imu_end beyond the samples", "imu_end negative"]
    for kind in kinds:
        tracks = [good[0], variant(kind), good[1], good[2]]
        filt = FU.new_filter(4)
        filt["p"][1] = (1.0, 2.0, 3.0)
        f, s, st, fo = _launch(torch, fu, filt, tracks)
        assert st == ARIA_E_INVALID, kind
        assert fu.status() == 0                                  # reported once
        assert f[1:2].tobytes() == filt[1:2].tobytes(), kind     # the filter is untouched
        bad = s[fo[1]:fo[2]]
        assert not bad["valid"].any() and not bad.tobytes().strip(b"\0"), kind
        keep = [0, 2, 3]
        assert f[keep].tobytes() == fg.tobytes(), kind
        assert np.concatenate([s[fo[k]:fo[k + 1]] for k in keep]).tobytes() == sg.tobytes(), kind
    # a negative count: an offset array that decreases. With its frame range intact the track's states are zeroed ...
    n0, n1 = len(good[0][0]), len(good[2][0])
    dummy = (np.zeros((0, 7)), np.zeros(5, np.int32), good[0][2][:5])
    f, s, st, fo = _launch(torch, fu, FU.new_filter(3), [good[0], good[2], dummy], ioff=[0, n0, n0 + n1, n0 + n1 - 3])
    assert st == ARIA_E_INVALID and f[2:3].tobytes() == FU.new_filter(1).tobytes() and not s[90:95].tobytes().strip(b"\0")
    assert f[0:1].tobytes() == fg[0:1].tobytes() and s[:60].tobytes() == sg[:60].tobytes()
    assert f[1:2].tobytes() == fg[2:3].tobytes() and s[60:90].tobytes() == sg[150:180].tobytes()
    # ... and with a frame range that decreases nothing of the track is written at all: its states keep the caller's bytes
    f, s, st, fo = _launch(torch, fu, FU.new_filter(2), [good[0], good[2]], foff=[0, 60, 50])
    assert st == ARIA_E_INVALID and f[1:2].tobytes() == FU.new_filter(1).tobytes()
    assert f[0:1].tobytes() == fg[0:1].tobytes() and s[:60].tobytes() == sg[:60].tobytes()
    assert set(s[60:].tobytes()) == {0xAB}
    # the host form reports the same and leaves the filter alone
    one = FU.new_filter(1)
    with pytest.raises(aria.AriaError) as ei:
        fu.run(*variant("nan sample"), one)
    assert ei.value.status == ARIA_E_INVALID and one.tobytes() == FU.new_filter(1).tobytes()


def test_edges_no_tracks_no_frames_no_imu(aria, fu, torch_cuda):
    from aria_slam_amd import fusion as FU
    from aria_slam_amd import fusion_ref as R
    torch = torch_cuda
    flt, states, status = fu.run_batch([])
    assert len(flt) == 0 and states == [] and status == 0
    imu, end, vis = _short("scene1", 30)
    empty = (np.zeros((0, 7)), np.zeros(0, np.int32), [])
    no_imu = (np.zeros((0, 7)), np.zeros(30, np.int32), vis)
    f, s, st, fo = _launch(torch, fu, FU.new_filter(3), [empty, no_imu, (imu, end, vis)])
    assert st == 0
    assert f[0:1].tobytes() == FU.new_filter(1).tobytes() and fo[1] == 0          # a track without frames: nothing happens
    ref = R.SensorFusion(np.longdouble)
    want = R.run_track(ref, *no_imu)                                              # updates only: P contracts
    got = s[fo[1]:fo[2]]
    assert got["valid"].all() and not got["n_predicted"].any() and got["n_updates"].sum() == 29
    assert _state_diff(got, want) <= 10 * GAP["scene1"][0]
    assert float(np.abs(f[1]["P"].reshape(15, 15) - ref.P).max() / np.abs(ref.P).max()) <= 10 * GAP["scene1"][1]
    # frames whose visual record is never accepted: the filter never starts, every sample is ignored
    never = (imu, end, [(t, Rm, p, 0) for t, Rm, p, _a in vis])
    one = FU.new_filter(1)
    st = fu.run(*never, one)
    assert one[0]["initialized"] == 0 and st["n_ignored"].sum() == len(imu) and not st["initialized"].any() and st["valid"].all()
    assert np.array_equal(one[0]["P"], FU.new_filter(1)[0]["P"])


def test_visual_from_pose_and_the_device_resident_chain(aria, fu, torch_cuda):
    from aria_slam_amd import _lib
    from aria_slam_amd import fusion as FU
    torch = torch_cuda
    imu, end, vis = _short("relpose", 100)
    rng = np.random.default_rng(0)
    pose = np.zeros(len(vis), _lib.POSE_RESULT_DTYPE)
    for k, (t, Rm, p, _a) in enumerate(vis):
        pose[k]["R"], pose[k]["t"] = np.asarray(Rm).reshape(9), p
    pose["E"] = rng.normal(size=(len(vis), 9))
    pose["n_pose_inliers"] = rng.integers(0, 30, len(vis))
    pose["valid"] = rng.integers(0, 8, len(vis)) > 0
    pose["n_pose_inliers"][0], pose["valid"][0] = 50, 1
    ts = np.array([v[0] for v in vis])
    d_pose, d_ts = _dev(torch, pose), _dev(torch, ts)
    d_vis = torch.zeros((len(vis) + 1) * _lib.FUSE_VISUAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fu.visual_from_pose_device(d_pose, d_ts, len(vis), 10, d_vis)
    fu.check()
    got = np.frombuffer(d_vis.cpu().numpy().tobytes(), _lib.FUSE_VISUAL_DTYPE)[:len(vis)]
    want = np.zeros(len(vis), _lib.FUSE_VISUAL_DTYPE)
    want["t"], want["R"], want["p"] = ts, pose["R"], pose["t"]
    want["accept"] = (pose["valid"] != 0) & (pose["n_pose_inliers"] > 10)
    assert got.tobytes() == want.tobytes() and 10 < want["accept"].sum() < len(vis)
    # pose -> fuse on what lies in HBM (same stream: no synchronisation in between) equals the host-fed run bit for bit
    track = (imu, end, want)
    fh, sh, st, _ = _launch(torch, fu, FU.new_filter(1), [track])
    d_vis.zero_()
    torch.cuda.synchronize()
    fu.visual_from_pose_device(d_pose, d_ts, len(vis), 10, d_vis)
    fd, sd, st2, _ = _launch(torch, fu, FU.new_filter(1), [track], vis_dev=d_vis)
    assert st == 0 and st2 == 0 and fd.tobytes() == fh.tobytes() and sd.tobytes() == sh.tobytes()
    assert sh["n_updates"].sum() == want["accept"].sum() - 1


def test_python_class_follows_the_reference_surface(aria):
    from aria_slam_amd import fusion_ref as R
    imu, end, vis = make_track("scene2")
    end, vis = end[:50], vis[:50]
    dev = aria.HipSensorFusion()
    ref = R.SensorFusion(np.longdouble)
    dev.add_imu(imu[0, 0] - 1.0, imu[0, 1:4], imu[0, 4:7])          # before the first pose: ignored by both
    ref.add_imu(imu[0, 0] - 1.0, imu[0, 1:4], imu[0, 4:7])
    assert not dev.is_initialized()
    i = 0
    for f in range(len(vis)):
        while i < end[f]:
            dev.add_imu(imu[i, 0], imu[i, 1:4], imu[i, 4:7])
            ref.add_imu(imu[i, 0], imu[i, 1:4], imu[i, 4:7])
            i += 1
        dev.add_visual_pose(*vis[f][:3])
        ref.add_visual_pose(*vis[f][:3])
        if f in (0, 10, 11, 49):                                     # a getter flushes: any chunking gives the same filter
            gs = GAP["scene2"][0]
            assert np.abs(dev.get_position() - ref.get_position()).max() <= 10 * gs
            assert np.abs(dev.get_velocity() - ref.get_velocity()).max() <= 10 * gs
            assert np.abs(dev.get_orientation() - ref.get_orientation()).max() <= 10 * gs
            assert np.abs(dev.get_bias()[0] - ref.get_bias()[0]).max() <= 10 * gs
            assert float(np.abs(dev.get_covariance() - ref.get_covariance()).max() / np.abs(ref.P).max()) <= 10 * GAP["scene2"][1]
    # trailing samples without a pose are consumed too
    for k in range(i, i + 5):
        dev.add_imu(imu[k, 0], imu[k, 1:4], imu[k, 4:7])
        ref.add_imu(imu[k, 0], imu[k, 1:4], imu[k, 4:7])
    assert np.abs(dev.get_position() - ref.get_position()).max() <= 10 * GAP["scene2"][0]
    assert dev.is_initialized() and dev.last_states["n_predicted"].sum() == 5
    imu = imu[:int(end[-1])]
    one = aria.HipSensorFusion()
    batch_f, batch_s, _ = one.run_batch([(imu, end, vis)])
    again = aria.HipSensorFusion()
    assert again.run(imu, end, vis).tobytes() == batch_s[0].tobytes() and again.filter.tobytes() == batch_f.tobytes()
    for o in (dev, one, again):
        o.close()


def test_cpp_adapter_equals_the_python_class(aria, tmp_path):
    """tests/cpp/fuse_selftest.cpp drives HipSensorFusion through the ISensorFusion port; the same events through the Python
    class give the same bits (the same library on the same arrays; chunking does not matter)."""
    from aria_slam_amd import fusion_ref as R
    imu, end, vis = make_track("scene3")
    end, vis = end[:40], vis[:40]
    lines, py = [], aria.HipSensorFusion()
    want = []

    def getter():
        lines.append("G")
        P = py.get_covariance()
        h = list(R.H_IDX)
        want.append(np.concatenate([[py.filter[0]["last_imu_time"]], py.get_position(), py.get_orientation(), py.get_velocity(),
                                    np.diag(P[np.ix_(h, h)]), [P[0, 7]], [float(py.is_initialized())]]))

    getter()                                                       # nothing queued: the constructor's state
    i = 0
    for f in range(len(vis)):
        while i < end[f]:
            lines.append("I " + " ".join(repr(float(x)) for x in imu[i]))
            py.add_imu(imu[i, 0], imu[i, 1:4], imu[i, 4:7])
            i += 1
        t, Rm, p, _a = vis[f]
        q = R.quat_from_rot(np.asarray(Rm))
        lines.append("V %r " % float(t) + " ".join(repr(float(x)) for x in list(q) + list(p)))
        py.add_visual_pose(t, R.quat_to_rot(q), p)                 # the adapter hands the filter R(q)
        if f in (0, 1, 17, 39):
            getter()
    for k in range(i, i + 3):                                      # trailing samples, then a getter
        lines.append("I " + " ".join(repr(float(x)) for x in imu[k]))
        py.add_imu(imu[k, 0], imu[k, 1:4], imu[k, 4:7])
    getter()
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines + ["R", "G", "P 5.0 0.5 0.5 0.5 0.5 1.0 2.0 3.0", "G"]) + "\n")
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    exe = os.path.join(ROOT, "build", "fuse_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "fuse_selftest.cpp"), "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    got = [np.array(l.split()[1:], np.float64) for l in out.stdout.splitlines() if l.startswith("state ")]
    assert len(got) == len(want) + 2
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes(), (a, b)
    assert got[0][-1] == 0 and got[1][-1] == 1 and list(got[0][1:8]) == [0, 0, 0, 1, 0, 0, 0]
    assert got[-2].tobytes() == got[0].tobytes()                    # reset()
    assert list(got[-1][:8]) == [5.0, 1.0, 2.0, 3.0, 0.5, 0.5, 0.5, 0.5] and got[-1][-1] == 1 and not got[-1][8:11].any()
    py.close()


def _tum_pose(row):
    from aria_slam_amd import fusion_ref as R
    T = np.eye(4)
    T[:3, :3] = R.quat_to_rot(R.quat_normalize(np.array([row[7], row[4], row[5], row[6]])))
    T[:3, 3] = row[1:4]
    return T


def test_euroc_frontend_fuse(aria, tmp_path):
    """--fuse FILE on a synthetic ASL tree with imu0: refused without --pose; the --pose file and the CSV are byte-identical
    with and without the flag; one TUM line per frame that equals the Python class fed with the same events. The events'
    relative poses are recovered from consecutive lines of the --pose file, which prints 9 decimals: the measurements are
    known to 5e-10 and, with gains below 1 and a velocity coupling of at most 1 / dt = 20 over the 15 updates, the two runs
    may differ by 1e-6 (metres, quaternion entries); that bound comes from the file format, not from the device."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_frontend_io import _make_dataset
    from test_fuse_host import write_imu_csv
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    seq, t0 = _make_dataset(aria, str(tmp_path), 8, w=640, h=480)
    n = len(seq)
    rng = np.random.default_rng(1)
    ts = [t0 - 20_000_000 + k * 5_000_000 for k in range(10 * n + 8)]
    rows = [(t,) + tuple(0.01 * rng.normal(size=3)) + tuple(np.array([0.0, 0.0, 9.81]) + 0.05 * rng.normal(size=3)) for t in ts]
    write_imu_csv(tmp_path, rows)
    exe = os.path.join(PKG, "euroc_frontend")
    p1, p2, c1, c2, f2 = (str(tmp_path / x) for x in ("p1.txt", "p2.txt", "c1.csv", "c2.csv", "fused.txt"))
    bad = subprocess.run([exe, str(tmp_path), "1000", "--fuse", f2], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--fuse needs --pose" in bad.stderr
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", p1, "--csv", c1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run([exe, str(tmp_path), "1000", "--pose", p2, "--csv", c2, "--fuse", f2], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(p1, "rb").read() == open(p2, "rb").read() and open(c1, "rb").read() == open(c2, "rb").read()
    line = [l for l in run.stdout.splitlines() if l.startswith("fused ")]
    assert len(line) == 1 and not [l for l in plain.stdout.splitlines() if l.startswith("fused ")]
    print(line[0])
    pose = np.array([l.split() for l in open(p2).read().splitlines()], np.float64)
    fused = np.array([l.split() for l in open(f2).read().splitlines()], np.float64)
    assert pose.shape == fused.shape == (n, 8) and np.array_equal(pose[:, 0], fused[:, 0])
    # the same events for the Python class: the reader's ranges (prev image < t <= image) and the accepted relative poses
    img_t = np.array([t0 + i * 50_000_000 for i in range(n)], np.int64)
    st = np.array(ts, np.int64)
    imu = np.array([[r[0] * 1e-9] + list(r[4:7]) + list(r[1:4]) for r in rows])
    end = np.array([int((st <= t).sum()) for t in img_t], np.int32)
    first = int((st <= 0).sum())
    assert first == 0
    vis = []
    for i in range(n):
        rel = np.linalg.inv(_tum_pose(pose[i - 1])) @ _tum_pose(pose[i]) if i else np.eye(4)
        accept = i > 0 and not np.array_equal(pose[i, 1:], pose[i - 1, 1:])
        vis.append((pose[i, 0], rel[:3, :3], rel[:3, 3], int(accept)))
    updates = int(line[0].split()[1])
    assert sum(v[3] for v in vis) - 1 == updates > 3
    py = aria.HipSensorFusion()
    stt = py.run(imu, end, vis)
    assert int(stt["n_updates"].sum()) == updates and int(stt["n_predicted"].sum()) == int(line[0].split()[7])
    d = max(np.abs(stt["p"] - fused[:, 1:4]).max(), np.abs(stt["q"][:, [1, 2, 3, 0]] - fused[:, 4:8]).max())
    print("euroc_frontend --fuse against the Python class: %.2e" % d)
    assert d <= 1e-6
    py.close()
