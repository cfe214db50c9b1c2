"""The case table of the fusion kernels' branches, shared by the CPU test (tests/test_fuse_host.py: it counts the branches
the restatement takes on every case, pins the margin of every decision and shows, on altered copies of the restatement, that
each case catches the mistake it is there for), the GPU test (tests/test_gpu_fuse_branches.py: the device against
fusion_ref in np.longdouble) and tools/fuse_gap.py (the tolerance table). A plain module: no fixtures, no pytest.

The eight tracks of tests/test_gpu_fuse.py never leave the neighbourhood of R = I: every quat_from_rot takes the trace
branch, every error quaternion has w > 0.99. The cases here reach what those leave out. track(name) gives
Track(imu (N, 7), imu_end (F,), visual [(t, R, p, accept)], edits, gravity): `edits` are changes to the filter record the
track starts from (keys: initialized, last_imu_time, last_visual_time, p, q, P = ((row, col, value), ...), noise = {name:
value}); ref_filter and record turn them into a fusion_ref.SensorFusion and a FUSE_FILTER_DTYPE record.

  turn_z      fusion_ref.make_scene(**TURN): the body yaws with the tangent through a full circle in 4 s, 81 frames, 800
              samples. 54 measurements take the trace branch, 27 the z-largest one; 47 of 80 error quaternions have w < 0,
              because quat_from_rot does not force a sign while the integrated orientation is continuous.
  turn_x      turn_z conjugated by the cyclic permutation W that sends z to x (p' = W p, R' = W R W^T, accel' = W accel,
  turn_y      gyro' = W gyro, gravity W g), and by the one that sends z to y. A permutation moves entries without rounding
              them: the same turn lands in the x-largest and the y-largest branch, and gravity lies along x and along y.
  turn_epoch  turn_z with t0 = 1403636580 s (EuRoC's epoch): timestamps with a grain of 2.4e-7 s, as on recorded data.
  ties_*      six frames, no samples, every frame measuring exactly the same R and p, one track per rotation of TIES. Every
              entry is 0 or +-1: the branch is decided by the order of the comparisons alone, in any precision. Frame 0
              initialises; frames 1..5 see an innovation rotation that is 0 (n == 0 in the log map) or a few ulps
              (angle < 1e-10 in the update). The issue lists the half turns about the axes, about (1,1,0), (0,1,1), (1,0,1)
              and the 120 degree turn about (1,1,1). On those every branch a tie could fall into gives the SAME quaternion:
              all components that could lead are positive. So four more were added, on which the other side of each
              comparison gives -q: the half turns about (1,-1,0), (0,1,-1), (1,0,-1) (one per pair of diagonal entries)
              and a 120 degree turn whose w is negative (trace exactly 0 against the x-largest branch).
  notpd_a/b/c a record with initialized = 1 whose covariance fails the Cholesky of the first frame's update, reached with
              no sample in between: (a) P[0][0] = -1, the first pivot; (b) P[6][6] = -1, the pivot of measured row 3 after
              three good ones; (c) P[0][0] = -pos_noise^2, a pivot of exactly 0. For (c) pos_noise is 2^-7, so that its
              square is the same number in fp64 and in the extended run. The frame leaves the state and P alone, counts
              no update and moves last_visual_time; the frames after it, with samples in between, run as on any track.
  zero_gyro   every gyro sample between frame 0 and frame 1 is exactly 0 and frame 1 is not accepted: bg is still 0, the
              step's angle is 0, and the orientation of frame 1 has the bits of frame 0. The accelerations are the scene's.
  resume      a record with initialized = 1 and last_imu_time = -1. Frame 0 holds one sample and no measurement: the sample
              only sets the time (n_skipped = 1), state and P keep their bits.

BRANCH_CASE names, for every branch of the census, the case that is there for it.

GAP[name] = (states, P relative), measured by tools/fuse_gap.py by the rule of tests/test_gpu_fuse.py: the restatement in
fp64 against itself in np.longdouble, states absolute, P relative to its largest entry. allowed(name) is ten times the
row, and ten times scene1's row where a case measures less (the static cases measure almost nothing). PREINT_GAP holds
the rows of the three interval kinds of preint_case; allowed_preint is ten times the row, with no floor."""
import collections
import functools

import numpy as np

from aria_slam_amd import fusion_ref as R

Track = collections.namedtuple("Track", "imu imu_end visual edits gravity")

TURN = dict(seed=22, duration=4.0, period=4.0, yaw_follows=True)
EPOCH = 1403636580.0
PERM = {"turn_x": (2, 0, 1), "turn_y": (1, 2, 0)}       # v'[a] = v[perm[a]]: W sends the z axis to x, and to y
TURNING = ("turn_z", "turn_x", "turn_y", "turn_epoch")

TIES = {
    "ties_x": ((1, 0, 0), (0, -1, 0), (0, 0, -1)),         # half turns about the axes, trace -1
    "ties_y": ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    "ties_z": ((-1, 0, 0), (0, -1, 0), (0, 0, 1)),
    "ties_xy": ((0, 1, 0), (1, 0, 0), (0, 0, -1)),         # half turns about (1,1,0), (0,1,1), (1,0,1): two diagonals tie at 0
    "ties_yz": ((-1, 0, 0), (0, 0, 1), (0, 1, 0)),
    "ties_zx": ((0, 0, 1), (0, -1, 0), (1, 0, 0)),
    "ties_111": ((0, 0, 1), (1, 0, 0), (0, 1, 0)),         # 120 degrees about (1,1,1): trace 0, all diagonals equal
    "ties_xny": ((0, -1, 0), (-1, 0, 0), (0, 0, -1)),      # half turns about (1,-1,0), (0,1,-1), (1,0,-1): the other side of
    "ties_ynz": ((-1, 0, 0), (0, 0, -1), (0, -1, 0)),      # the tie gives -q
    "ties_xnz": ((0, 0, -1), (0, -1, 0), (-1, 0, 0)),
    "ties_111n": ((0, 0, -1), (1, 0, 0), (0, -1, 0)),      # 120 degrees, w = -1/2: the trace branch would give -q
}
NOTPD = {"notpd_a": ((0, 0, -1.0),), "notpd_b": ((6, 6, -1.0),), "notpd_c": ((0, 0, -2.0 ** -14),)}
NAMES = list(TURNING) + list(TIES) + list(NOTPD) + ["zero_gyro", "resume"]

BRANCH_CASE = {
    "qfr_trace": "turn_z", "qfr_x": "turn_x", "qfr_y": "turn_y", "qfr_z": "turn_z",
    "log_w_pos": "turn_z", "log_w_neg": "turn_z", "log_n_zero": "ties_111",
    "predict_turns": "turn_z", "predict_zero_angle": "zero_gyro",
    "update_turns": "turn_z", "update_zero_angle": "ties_111",
    "notpd_first_pivot": "notpd_a", "notpd_later_pivot": "notpd_b", "notpd_zero_pivot": "notpd_c",
    "resume_skip": "resume",
}
# what the tracks of tests/test_gpu_fuse.py visit; the census asserts they visit nothing else
OLD_BRANCHES = {"qfr_trace", "log_w_pos", "predict_turns", "update_turns"}

# ---- the output of tools/fuse_gap.py, copied
GAP = {
    "turn_z": (6.56e-15, 1.36e-14),
    "turn_x": (6.40e-15, 1.46e-14),
    "turn_y": (5.66e-15, 1.39e-14),
    "turn_epoch": (5.64e-15, 4.25e-15),
    "ties_x": (0.00e+00, 7.26e-19),
    "ties_y": (0.00e+00, 7.26e-19),
    "ties_z": (0.00e+00, 7.26e-19),
    "ties_xy": (6.27e-17, 7.26e-19),
    "ties_yz": (6.27e-17, 7.26e-19),
    "ties_zx": (6.27e-17, 7.26e-19),
    "ties_111": (0.00e+00, 7.26e-19),
    "ties_xny": (6.27e-17, 7.26e-19),
    "ties_ynz": (6.27e-17, 7.26e-19),
    "ties_xnz": (6.27e-17, 7.26e-19),
    "ties_111n": (0.00e+00, 7.26e-19),
    "notpd_a": (5.32e-16, 2.80e-15),
    "notpd_b": (5.32e-16, 2.11e-15),
    "notpd_c": (2.69e-14, 5.64e-15),
    "zero_gyro": (2.62e-15, 9.81e-15),
    "resume": (2.63e-15, 9.89e-15),
}
PREINT_GAP = {
    "zero_angle": (3.22e-16, 9.00e-16),
    "full_turn": (7.85e-14, 2.51e-15),
    "epoch": (3.00e-14, 3.19e-15),
}
GAP_FLOOR = (4.88e-15, 7.40e-15)           # scene1's row of tests/test_gpu_fuse.py


def allowed(name):
    return tuple(10 * max(g, f) for g, f in zip(GAP[name], GAP_FLOOR))


def allowed_preint(kind):
    return tuple(10 * g for g in PREINT_GAP[kind])


# ---- the tracks
def _scene(**kw):
    sc = R.make_scene(**kw)
    return sc["imu"], sc["imu_end"], sc["visual"]


def _started(vis0, **more):
    """Edits of a record that has seen `vis0` as its first pose."""
    t, Rm, p, _a = vis0
    e = dict(initialized=1, last_imu_time=t, last_visual_time=t, p=tuple(p), q=tuple(R.quat_from_rot(np.asarray(Rm, np.float64))))
    e.update(more)
    return e


@functools.lru_cache(maxsize=None)
def track(name):
    g = R.DEFAULT_GRAVITY
    if name == "turn_z":
        return Track(*_scene(**TURN), {}, g)
    if name == "turn_epoch":
        return Track(*_scene(t0=EPOCH, **TURN), {}, g)
    if name in PERM:
        imu, end, vis = _scene(**TURN)
        pm = list(PERM[name])
        imu = np.concatenate([imu[:, :1], imu[:, 1:4][:, pm], imu[:, 4:7][:, pm]], axis=1)
        vis = [(t, np.asarray(Rm)[np.ix_(pm, pm)].copy(), np.asarray(p)[pm].copy(), a) for t, Rm, p, a in vis]
        return Track(imu, end, vis, {}, tuple(np.array(g)[pm]))
    if name in TIES:
        Rm, p = np.array(TIES[name], np.float64), np.array([0.5, -0.25, 2.0])
        return Track(np.zeros((0, 7)), np.zeros(6, np.int32), [(100.0 + 0.05 * f, Rm, p, 1) for f in range(6)], {}, g)
    if name in NOTPD:
        imu, end, vis = _scene(seed=23, duration=0.5)               # 11 frames, 100 samples; frame 0 has none before it
        more = dict(noise=dict(pos_noise=2.0 ** -7)) if name == "notpd_c" else {}
        # last_visual_time lies before the first frame, so that the rejected measurement is seen to move it
        return Track(imu, end, vis, _started(vis[0], P=NOTPD[name], last_visual_time=vis[0][0] - 0.05, **more), g)
    if name == "zero_gyro":
        imu, end, vis = _scene(seed=24, duration=1.0, period=4.0, yaw_follows=True)
        imu = imu.copy()
        imu[:int(end[1]), 4:7] = 0.0
        vis = list(vis)
        vis[1] = vis[1][:3] + (0,)
        return Track(imu, end, vis, {}, g)
    assert name == "resume", name
    imu, end, vis = _scene(seed=25, duration=1.0, period=4.0, yaw_follows=True)
    end = end.copy()
    end[0] = 1
    edits = _started(vis[0], last_imu_time=-1.0)
    vis = [vis[0][:3] + (0,)] + list(vis[1:])
    return Track(imu, end, vis, edits, g)


def ref_filter(tr, dtype=np.float64, mod=R):
    """The fusion_ref.SensorFusion (of `mod`, a copy of the restatement, where given) a track starts from."""
    e = tr.edits
    flt = mod.SensorFusion(dtype, gravity=tr.gravity, **e.get("noise", {}))
    T = flt.dtype.type
    if "p" in e:
        flt.position = np.array(e["p"], dtype=flt.dtype)
    if "q" in e:
        flt.orientation = np.array(e["q"], dtype=flt.dtype)
    for r, c, v in e.get("P", ()):
        flt.P[r, c] = T(v)
    if "last_imu_time" in e:
        flt.last_imu_time = T(e["last_imu_time"])
    if "last_visual_time" in e:
        flt.last_visual_time = T(e["last_visual_time"])
    flt.initialized = bool(e.get("initialized", 0))
    return flt


def record(tr):
    """The FUSE_FILTER_DTYPE record (one element) a track starts from."""
    from aria_slam_amd import fusion as FU
    return FU.filter_from_ref(ref_filter(tr))


@functools.lru_cache(maxsize=None)
def ref_runs(name):
    """(fp64 states, fp64 filter, extended states, extended filter) of the restatement on a case. Shared: do not modify."""
    tr = track(name)
    f64, fld = ref_filter(tr), ref_filter(tr, np.longdouble)
    return (R.run_track(f64, tr.imu, tr.imu_end, tr.visual), f64, R.run_track(fld, tr.imu, tr.imu_end, tr.visual), fld)


STATE_KEYS = ("p", "v", "q", "ba", "bg")
COUNTERS = ("n_predicted", "n_skipped", "n_ignored", "n_updates", "initialized")
FILTER_ATTRS = ("position", "velocity", "orientation", "accel_bias", "gyro_bias")


def measure_gap(name):
    """(states, P relative) between the fp64 and the extended run, by the rule of tools/fuse_gap.py."""
    s64, f64, sld, fld = ref_runs(name)
    gs = max(float(np.abs(s64[k] - sld[k]).max()) for k in STATE_KEYS)
    gs = max(gs, max(float(np.abs(getattr(f64, a) - getattr(fld, a)).max()) for a in FILTER_ATTRS))
    gp = float(np.abs(f64.P - fld.P).max() / np.abs(fld.P).max())
    gd = float(np.abs(s64["P_diag"] - sld["P_diag"]).max() / np.abs(sld["P_diag"]).max())
    for k in COUNTERS:
        assert np.array_equal(s64[k], sld[k]), (name, k)
    return gs, max(gp, gd)


# ---- preintegration
PREINT_KINDS = ("zero_angle", "full_turn", "epoch")
PREINT_BIAS = np.array([0.05, -0.03, 0.02, 2.0 ** -9, -(2.0 ** -10), 3 * 2.0 ** -11])     # the gyro part is a short dyadic triple


@functools.lru_cache(maxsize=None)
def preint_case(kind):
    """(imu, begin, end, bias) of an interval kind. Shared: do not modify.
    zero_angle  forty intervals of twenty samples of turn_z; in the first ten every gyro sample EQUALS the gyro bias: the
                step's angle is exactly 0, delta_q stays (1, 0, 0, 0) and the orientation block of the covariance still grows
    full_turn   one interval over all 800 samples of turn_z: delta_q.w crosses 0 and ends negative
    epoch       all of turn_epoch, and its eight hundreds"""
    if kind == "zero_angle":
        imu = track("turn_z").imu.copy()
        imu[:200, 4:7] = PREINT_BIAS[3:6]
        begin = 20 * np.arange(40, dtype=np.int32)
        return imu, begin, begin + 20, PREINT_BIAS
    if kind == "full_turn":
        return track("turn_z").imu, np.array([0], np.int32), np.array([800], np.int32), PREINT_BIAS
    assert kind == "epoch", kind
    begin = np.array([0] + [100 * k for k in range(8)], np.int32)
    end = np.array([800] + [100 * (k + 1) for k in range(8)], np.int32)
    return track("turn_epoch").imu, begin, end, PREINT_BIAS


@functools.lru_cache(maxsize=None)
def preint_refs(kind):
    """(fp64, extended) results of fusion_ref.preintegrate on an interval kind. Shared: do not modify."""
    imu, begin, end, bias = preint_case(kind)
    return R.preintegrate(imu, begin, end, bias), R.preintegrate(imu, begin, end, bias, dtype=np.longdouble)


def measure_preint_gap(kind):
    a, b = preint_refs(kind)
    gs = max(float(np.abs(a[k] - b[k]).max()) for k in ("delta_p", "delta_v", "delta_q", "dt_sum"))
    return gs, float(np.abs(a["cov"] - b["cov"]).max() / np.abs(b["cov"]).max())
