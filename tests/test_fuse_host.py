"""Visual-inertial fusion (include/aria_orb_hip.h, "visual-inertial fusion"): the parts that need no GPU -- exports and record
layouts, known answers of the NumPy restatement (aria_slam_amd/fusion_ref.py) that do not go through its own code path, its
behaviour on the scene generator, the kernels' listing, and the case table of the kernels' branches (tests/fuse_cases.py): a
census of the branches the restatement takes on it, the margin of every decision, and altered copies of the restatement that
each case must catch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

FUSE_SYMBOLS = ["aria_fuse_default_config", "aria_fuse_create", "aria_fuse_destroy", "aria_fuse_stream", "aria_fuse_check",
                "aria_fuse_filter_init", "aria_fuse_run_batch_device", "aria_fuse_run", "aria_fuse_visual_from_pose_device",
                "aria_fuse_preintegrate_batch_device", "aria_fuse_preintegrate"]
RECORDS = ["aria_fuse_config", "aria_imu_sample", "aria_fuse_visual", "aria_fuse_filter", "aria_fuse_state", "aria_preint_result"]


def test_fuse_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in FUSE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipSensorFusion and aria.HipImuPreintegrator


def test_fuse_record_layouts_and_defaults(aria, tmp_path):
    from aria_slam_amd import _lib
    from aria_slam_amd import fusion as FU
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aria_orb_hip.h"\nint main(void) { printf("' + "%zu " * len(RECORDS) + '\\n", ' +
                   ", ".join("sizeof(%s)" % r for r in RECORDS) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [88, 56, 112, 2024, 280, 744]
    assert C.sizeof(_lib.FuseConfig) == 88
    for struct, dtype, size in ((_lib.ImuSample, _lib.IMU_SAMPLE_DTYPE, 56), (_lib.FuseVisual, _lib.FUSE_VISUAL_DTYPE, 112),
                                (_lib.FuseFilter, _lib.FUSE_FILTER_DTYPE, 2024), (_lib.FuseState, _lib.FUSE_STATE_DTYPE, 280),
                                (_lib.PreintResult, _lib.PREINT_RESULT_DTYPE, 744)):
        assert C.sizeof(struct) == dtype.itemsize == size
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
    # the defaults of include/legacy/IMU.hpp:105-113 and the constructor's P0 (src/legacy/IMU.cpp:104-111)
    cfg = _lib.FuseConfig()
    aria.load_library().aria_fuse_default_config(C.byref(cfg))
    assert cfg.struct_size == 88 and list(cfg.gravity) == [0.0, 0.0, -9.81]
    assert (cfg.accel_noise, cfg.gyro_noise, cfg.accel_bias_walk, cfg.gyro_bias_walk, cfg.pos_noise, cfg.rot_noise) == \
        (0.1, 0.01, 0.001, 0.0001, 0.01, 0.01)
    f = FU.new_filter(2, accel_noise=0.2)[1]
    assert np.array_equal(f["P"].reshape(15, 15), np.diag([0.01] * 9 + [0.001] * 3 + [0.0001] * 3))
    assert list(f["q"]) == [1, 0, 0, 0] and f["last_imu_time"] == -1 and f["last_visual_time"] == -1 and f["initialized"] == 0
    assert f["accel_noise"] == 0.2 and f["gyro_noise"] == 0.01 and list(f["gravity"]) == [0, 0, -9.81]
    assert not f["p"].any() and not f["v"].any() and not f["ba"].any() and not f["bg"].any()
    # the restatement starts from the same record
    from aria_slam_amd import fusion_ref as R
    assert FU.filter_from_ref(R.SensorFusion(accel_noise=0.2)).tobytes() == f.tobytes()


# ---- known answers of the restatement ---------------------------------------------------------------------------------------
def _started(R, t=10.0, Rm=np.eye(3), p=(0, 0, 0), **kw):
    f = R.SensorFusion(**kw)
    f.add_visual_pose(t, Rm, p)
    return f


def test_at_rest_nothing_moves_and_p_grows_by_the_closed_form():
    from aria_slam_amd import fusion_ref as R
    f = _started(R)
    dt = 0.005
    f.add_imu(10.0 + dt, (0, 0, 9.81), (0, 0, 0))
    assert not f.position.any() and not f.velocity.any() and list(f.orientation) == [1, 0, 0, 0]
    P = f.P
    d2, g = dt * dt, 9.81
    want = {(12, 12): 1e-4 + d2 * 1e-8,                                   # bias walk
            (9, 9): 1e-3 + d2 * 1e-6,
            (6, 6): 0.01 + d2 * 1e-4 + d2 * 1e-4,                         # gyro bias variance and gyro noise
            (5, 5): 0.01 + d2 * 1e-3 + d2 * 0.01,                         # vz: accel bias and accel noise; skew(a) has no z row
            (3, 3): 0.01 + (g * dt) ** 2 * 0.01 + d2 * 1e-3 + d2 * 0.01,  # vx: tilt about y couples gravity in
            (2, 2): 0.01 + d2 * 0.01 + 0.25 * d2 * d2 * 1e-3 + 0.25 * d2 * d2 * 0.01}
    for (r, c), w in want.items():       # a dozen fp64 operations on either side, each within 2^-53: 16 of them at most
        assert abs(P[r, c] - w) <= 16 * 2.0 ** -53 * abs(w), ((r, c), P[r, c], w)
    assert np.array_equal(P, P.T)


def test_constant_acceleration_and_constant_yaw_rate():
    from aria_slam_amd import fusion_ref as R
    f = _started(R)
    dt, n = 0.005, 400
    for k in range(1, n + 1):
        f.add_imu(10.0 + k * dt, (1.0, -0.5, 9.81 + 0.25), (0, 0, 0))
    T = n * dt
    a = np.array([1.0, -0.5, 0.25])
    # p += v dt + a dt^2 / 2 is exact for a constant acceleration: only rounding is left
    assert np.abs(f.velocity - a * T).max() < 1e-13 and np.abs(f.position - 0.5 * a * T * T).max() < 1e-13
    f = _started(R)
    w = 0.7
    for k in range(1, n + 1):
        f.add_imu(10.0 + k * dt, (0, 0, 9.81), (0, 0, w))
    q = f.orientation
    assert abs(q[0] - np.cos(0.5 * w * T)) < 1e-13 and abs(q[3] - np.sin(0.5 * w * T)) < 1e-13 and abs(q[1]) + abs(q[2]) < 1e-15
    assert np.abs(f.position).max() < 1e-13        # gravity keeps cancelling while the body yaws about it


def _literal_F_G(Rm, a, dt):
    """F and G written block by block from src/legacy/IMU.cpp:179-213, with loops instead of the restatement's slices."""
    Sk = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    RS = [[sum(Rm[i][k] * Sk[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    F = [[1.0 if i == j else 0.0 for j in range(15)] for i in range(15)]
    G = [[0.0] * 12 for _ in range(15)]
    for i in range(3):
        F[i][3 + i] = dt
        F[6 + i][12 + i] = -dt
        G[6 + i][3 + i] = dt
        G[9 + i][6 + i] = dt
        G[12 + i][9 + i] = dt
        for j in range(3):
            F[i][6 + j] = -0.5 * RS[i][j] * dt * dt
            F[i][9 + j] = -0.5 * Rm[i][j] * dt * dt
            F[3 + i][6 + j] = -RS[i][j] * dt
            F[3 + i][9 + j] = -Rm[i][j] * dt
            G[i][j] = 0.5 * Rm[i][j] * dt * dt
            G[3 + i][j] = Rm[i][j] * dt
    return np.array(F), np.array(G)


def test_F_and_G_entry_by_entry_and_against_central_differences():
    from aria_slam_amd import fusion_ref as R
    rng = np.random.default_rng(5)
    q = R.quat_normalize(rng.normal(size=4))
    Rm = R.quat_to_rot(q)
    a, w, dt = rng.normal(size=3) * 3 + [0, 0, 9.81], rng.normal(size=3) * 0.5, 0.005
    F, G = R.predict_jacobians(Rm, a, dt)
    F2, G2 = _literal_F_G(Rm.tolist(), a.tolist(), dt)
    assert np.abs(F - F2).max() < 1e-18 + 4e-16 * np.abs(F2).max() and np.array_equal(F != 0, F2 != 0)
    assert np.abs(G - G2).max() < 1e-18 + 4e-16 * np.abs(G2).max() and np.array_equal(G != 0, G2 != 0)
    assert np.count_nonzero(F - np.eye(15)) == 3 + 9 * 4 + 3 and np.count_nonzero(G) == 9 * 2 + 9

    # the state prediction as a function of (p, v, theta [a RIGHT perturbation of q], ba, bg)
    def predict(x):
        f = _started(R, Rm=Rm)
        f.orientation = R.quat_normalize(R.quat_mul(q, R.exp_map(x[6:9].copy())))
        f.position, f.velocity, f.accel_bias, f.gyro_bias = x[0:3].copy(), x[3:6].copy(), x[9:12].copy(), x[12:15].copy()
        f.add_imu(10.0 + dt, a, w)
        return np.concatenate([f.position, f.velocity])

    x0 = np.concatenate([rng.normal(size=6), np.zeros(3), rng.normal(size=3) * 0.05, rng.normal(size=3) * 0.01])
    h = 1e-5
    num = np.zeros((6, 15))
    for c in range(15):
        e = np.zeros(15)
        e[c] = h
        num[:, c] = (predict(x0 + e) - predict(x0 - e)) / (2 * h)
    F0, _ = R.predict_jacobians(Rm, a - x0[9:12], dt)
    # F's position and velocity rows ARE the Jacobian of the prediction with respect to p, v, a right-multiplied theta and ba
    # (central differences, h = 1e-5: truncation ~ h^2 |a| dt ~ 1e-11, rounding ~ 1e-16 / h ~ 1e-11 on entries <= 1)
    assert np.abs(num[:, 0:12] - F0[0:6, 0:12]).max() < 1e-9
    # F has zeros in the gyro-bias columns of those rows, and within one step that is exact too: R is taken before the gyro
    # step, so p and v do not feel bg. Where F is a model and NOT the Jacobian is the orientation rows: the true
    # d theta' / d theta is exp(-w dt) ~ I - skew(w dt), F says I (and -dt I for d theta' / d bg is first order only)
    assert np.abs(num[:, 12:15]).max() < 1e-9 and not F0[0:6, 12:15].any()
    assert np.array_equal(F0[6:9, 6:9], np.eye(3)) and np.linalg.norm(w * dt) > 1e-4


def test_update_gain_against_numpy_solve_and_joseph_is_spd():
    from aria_slam_amd import fusion_ref as R
    rng = np.random.default_rng(9)
    f = _started(R)
    A = rng.normal(size=(15, 15)) * 0.05
    f.P = A @ A.T + np.diag([0.01] * 15)
    f.position, f.velocity = rng.normal(size=3), rng.normal(size=3)
    f.orientation = R.quat_normalize(rng.normal(size=4))
    P0, p0, v0, q0 = f.P.copy(), f.position.copy(), f.velocity.copy(), f.orientation.copy()
    Rm = R.quat_to_rot(R.quat_normalize(R.quat_mul(R.exp_map(np.array([0.02, -0.01, 0.03])), q0)))
    pm = p0 + [0.01, 0.02, -0.015]
    f.add_visual_pose(11.0, Rm, pm)
    h = list(R.H_IDX)
    Sm = P0[np.ix_(h, h)] + np.diag([1e-4] * 6)
    innov = np.concatenate([pm - p0, [0.02, -0.01, 0.03]])
    dx = P0[:, h] @ np.linalg.solve(Sm, innov)
    assert np.abs(f.position - (p0 + dx[0:3])).max() < 1e-13 and np.abs(f.velocity - (v0 + dx[3:6])).max() < 1e-13
    assert np.abs(f.accel_bias - dx[9:12]).max() < 1e-13 and np.abs(f.gyro_bias - dx[12:15]).max() < 1e-13
    want_q = R.quat_normalize(R.quat_mul(R.exp_map(dx[6:9]), q0))          # left multiplication
    assert np.abs(f.orientation - want_q).max() < 1e-13
    K = np.linalg.solve(Sm, P0[:, h].T).T
    Hm = np.zeros((6, 15))
    Hm[range(6), h] = 1
    want_P = (np.eye(15) - K @ Hm) @ P0 @ (np.eye(15) - K @ Hm).T + K @ np.diag([1e-4] * 6) @ K.T
    assert np.abs(f.P - want_P).max() < 1e-14 * np.abs(P0).max()
    assert np.array_equal(f.P, f.P.T) and np.linalg.eigvalsh(f.P).min() > 0
    assert f.n_updates == 1 and f.last_visual_time == 11.0
    # a covariance that is not positive definite on the measured rows skips the update (a rule of ours)
    g = _started(R)
    g.P = -np.eye(15)
    before = (g.position.copy(), g.P.copy())
    g.add_visual_pose(11.0, Rm, pm)
    assert g.n_updates == 0 and np.array_equal(g.position, before[0]) and np.array_equal(g.P, before[1]) and g.last_visual_time == 11.0


def test_quaternion_conventions_and_log_map_corners():
    from aria_slam_amd import fusion_ref as R
    rng = np.random.default_rng(2)
    # every branch of quat_from_rot gives the rotation back; w's sign is not forced
    for axis, ang in (([1, 0, 0], 3.1), ([0, 1, 0], 3.1), ([0, 0, 1], 3.1), ([1, 2, 3], 0.3), ([1, 1, 0], np.pi), ([3, 2, 1], -3.0)):
        ax = np.array(axis, float) / np.linalg.norm(axis)
        Rm = R.rotvec_to_rot(ax * ang)
        q = R.quat_from_rot(Rm)
        assert abs(q @ q - 1) < 1e-14 and np.abs(R.quat_to_rot(q) - Rm).max() < 1e-14
    # the log map does not see the sign of q
    for _ in range(20):
        q = R.quat_normalize(rng.normal(size=4))
        assert np.array_equal(R.log_map(q), R.log_map(-q))
        th = R.log_map(q)
        assert np.linalg.norm(th) <= np.pi + 1e-15
        assert np.abs(R.quat_to_rot(R.exp_map(th)) - R.quat_to_rot(q)).max() < 1e-14
    assert not R.log_map(np.array([1.0, 0, 0, 0])).any() and not R.log_map(np.array([-1.0, 0, 0, 0])).any()
    ax = np.array([2.0, -1, 2]) / 3
    for th in (np.pi - 1e-9, np.pi - 1e-3):
        q = np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * ax])
        assert np.abs(R.log_map(q) - th * ax).max() < 1e-14
        assert np.abs(R.log_map(-q) - th * ax).max() < 1e-14
    # just past the half turn the angle folds back: the axis flips, the rotation is the same
    q = np.concatenate([[np.cos((np.pi + 1e-3) / 2)], np.sin((np.pi + 1e-3) / 2) * ax])
    assert np.abs(R.log_map(q) + (np.pi - 1e-3) * ax).max() < 1e-12


def test_every_skip_rule():
    from aria_slam_amd import fusion_ref as R
    f = R.SensorFusion()
    f.add_imu(9.0, (1, 2, 3), (0.1, 0.2, 0.3))                 # before initialisation: nothing, not even the time
    assert f.n_ignored == 1 and f.last_imu_time == -1 and not f.position.any() and not f.is_initialized()
    Rm = R.rotvec_to_rot(np.array([0.1, 0.2, -0.3]))
    f.add_visual_pose(10.0, Rm, (1, 2, 3))                     # the first pose initialises and returns
    assert f.is_initialized() and list(f.position) == [1, 2, 3] and f.last_imu_time == 10.0 and f.last_visual_time == 10.0
    assert f.n_updates == 0 and np.array_equal(f.orientation, R.quat_from_rot(Rm)) and np.array_equal(np.diag(f.P)[:3], [0.01] * 3)
    snap = lambda: (f.position.copy(), f.velocity.copy(), f.orientation.copy(), f.P.copy())
    s0 = snap()
    for t in (10.0, 9.5, 9.7 + 0.1 + 1e-9):                    # dt = 0, dt < 0, dt > 0.1 against the moved time
        f.add_imu(t, (1, 2, 3), (0.1, 0.2, 0.3))
        assert f.last_imu_time == t and all(np.array_equal(a, b) for a, b in zip(s0, snap()))
    assert f.n_skipped == 3 and f.n_predicted == 0
    f.add_imu(f.last_imu_time + 0.1, (1, 2, 3), (0.1, 0.2, 0.3))   # dt = 0.1 exactly is taken (up to the sum's rounding)
    assert f.n_predicted + f.n_skipped == 4
    f.add_imu(f.last_imu_time + 0.05, (1, 2, 3), (0.1, 0.2, 0.3))
    assert f.n_predicted >= 1 and not np.array_equal(s0[0], f.position)
    # preintegrator: the first sample only sets the time; dt <= 0 and dt > 0.5 are skipped but move the time
    p = R.IMUPreintegrator()
    p.integrate(5.0, (1, 0, 0), (0, 0, 0.1))
    assert p.n_used == 0 and p.last_timestamp == 5.0 and p.dt_sum == 0 and not p.covariance.any()
    p.integrate(5.0, (1, 0, 0), (0, 0, 0.1))
    p.integrate(5.6, (1, 0, 0), (0, 0, 0.1))
    assert p.n_used == 0 and p.last_timestamp == 5.6 and not p.delta_p.any()
    p.integrate(6.1, (1, 0, 0), (0, 0, 0.1))                   # dt = 0.5 (rounded) is taken
    assert p.n_used == 1 and abs(p.dt_sum - 0.5) < 1e-15 and abs(p.delta_v[0] - 0.5) < 1e-15 and abs(p.delta_p[0] - 0.125) < 1e-15
    # a_w used delta_q BEFORE the rotation (identity: delta_v has no y part), the covariance's G the one AFTER it
    assert p.delta_v[1] == 0 and p.covariance[3, 4] != 0
    Rq = R.quat_to_rot(p.delta_q)
    assert abs(p.covariance[3, 3] - ((Rq[0] * 0.5) @ (Rq[0] * 0.5)) * 1e-4) < 1e-18
    assert abs(p.covariance[6, 6] - 0.25 * 1e-6) < 1e-20


def test_one_piece_or_chunks_give_identical_bits():
    from aria_slam_amd import fusion_ref as R
    sc = R.make_scene(4, duration=3.0)
    whole = R.SensorFusion()
    a = R.run_track(whole, sc["imu"], sc["imu_end"], sc["visual"])
    parts = R.SensorFusion()
    cuts = [0, 7, 8, 31, len(sc["visual"])]
    outs = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s0 = int(sc["imu_end"][lo - 1]) if lo else 0
        outs.append(R.run_track(parts, sc["imu"][s0:int(sc["imu_end"][hi - 1])], sc["imu_end"][lo:hi] - s0, sc["visual"][lo:hi]))
    for k in R.STATE_FIELDS:
        assert np.array_equal(a[k], np.concatenate([o[k] for o in outs])), k
    assert np.array_equal(whole.P, parts.P) and whole.last_imu_time == parts.last_imu_time


def test_fusion_beats_the_raw_measurements_on_the_scene():
    """A 2 m circle with a vertical wobble and a gently rocking body, 200 Hz IMU with bias and noise, a visual pose every 10
    samples with 1 cm / 5 mrad noise, 20 s: fused position RMSE at most 0.9 of the raw measurements' RMSE.

    Measured on this restatement (fused / raw, metres): seed 1 0.0077 / 0.0172 = 0.45, seed 2 0.0088 / 0.0175 = 0.50,
    seed 3 0.0088 / 0.0175 = 0.50; P's smallest eigenvalue ends at 2.7e-8. With make_scene(yaw_follows=True) -- the body
    turning through the full circle -- the same filter is WORSE than its measurements (ratios 3.1, 4.2, 3.2, noise-free
    input included): the reference's F treats the orientation error as a body-frame one (dv/dtheta = -R skew(a)) while its
    update measures and applies it in the world frame (log(q_meas q^-1), exp(dx) q); the two agree only near R = I. That
    is the reference's behaviour, restated and not repaired."""
    from aria_slam_amd import fusion_ref as R
    for seed in (1, 2, 3):
        sc = R.make_scene(seed)
        f = R.SensorFusion()
        out = R.run_track(f, sc["imu"], sc["imu_end"], sc["visual"])
        fused = np.sqrt(np.mean(np.sum((out["p"] - sc["truth_p"]) ** 2, 1)))
        raw = np.sqrt(np.mean(np.sum((sc["meas_p"] - sc["truth_p"]) ** 2, 1)))
        ev = np.linalg.eigvalsh(f.P).min()
        print("seed %d fused %.4f raw %.4f ratio %.3f min eig %.3g" % (seed, fused, raw, fused / raw, ev))
        assert fused <= 0.9 * raw, (seed, fused, raw)
        assert ev > 0 and int(out["n_updates"].sum()) == len(sc["visual"]) - 1 and int(out["n_predicted"].sum()) == len(sc["imu"])


def test_restatement_runs_in_extended_precision():
    from aria_slam_amd import fusion_ref as R
    sc = R.make_scene(1, duration=2.0)
    a = R.run_track(R.SensorFusion(), sc["imu"], sc["imu_end"], sc["visual"])
    fl = R.SensorFusion(np.longdouble)
    b = R.run_track(fl, sc["imu"], sc["imu_end"], sc["visual"])
    assert b["p"].dtype == np.longdouble and fl.P.dtype == np.longdouble
    gap = max(float(np.abs(a[k] - b[k]).max()) for k in ("p", "v", "q", "ba", "bg"))
    if np.finfo(np.longdouble).eps < 1e-18:
        assert 0 < gap < 1e-12          # the two runs differ, by rounding only
    pa = R.preintegrate(sc["imu"], [0, 10], [10, 40])
    pb = R.preintegrate(sc["imu"], [0, 10], [10, 40], dtype=np.longdouble)
    assert pb["cov"].dtype == np.longdouble and np.abs(pa["cov"] - pb["cov"]).max() < 1e-15 * np.abs(pa["cov"]).max() * 100


# ---- the kernels' listing and the build ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    path = str(tmp_path_factory.mktemp("fuse") / "imu_fusion.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "imu_fusion.hip")])
    return open(path).read()


@pytest.mark.parametrize("kernel", ["k_ekf_tracks", "k_imu_preintegrate", "k_visual_from_pose"])
def test_fuse_kernels_cross_compile_without_scratch(listing, kernel):
    body, meta = S.kernel_body(listing, kernel)
    assert len(body) > 30
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(listing, kernel)
    assert not in_loop and not outside
    assert meta.get("LDSByteSize", 0) <= 64 * 1024
    print(kernel, len(body), meta)


def test_imu_fusion_is_in_the_product_build_reads_no_environment_and_has_no_float_atomics():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "imu_fusion.hip" in src_line
    text = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "imu_fusion.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    text += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in text)
    assert "getenv" not in text and "atomicAdd" not in text
    assert "__syncthreads" not in text      # the recurrence has no workgroup barrier


# ---- C++: the adapter, the selftest driver, the reader ---------------------------------------------------------------------
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_reference_headers import REF_INC, needs_reference   # noqa: E402


def test_fuse_adapter_and_selftest_build(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True,
                          text=True, check=True).stdout
    for name in ("HipSensorFusion::predictIMU", "HipSensorFusion::updateVO", "HipSensorFusion::getFusedPose",
                 "HipSensorFusion::getVelocity", "HipSensorFusion::reset", "aria_asl_imu"):
        assert name in syms, name
    usage = subprocess.run([os.path.join(PKG, "euroc_frontend")], capture_output=True, text=True)
    assert "--fuse" in usage.stderr
    bad = subprocess.run([os.path.join(PKG, "euroc_frontend"), "/nonexistent", "--fuse", "x.txt"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--fuse needs --pose" in bad.stderr
    out = os.path.join(ROOT, "build", "fuse_selftest")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "fuse_selftest.cpp"), "-o", out, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])


@needs_reference
def test_fuse_adapter_compiles_against_the_reference_headers(tmp_path):
    """HipSensorFusion implements the reference's real interfaces::ISensorFusion (Eigen types through the test-only stand-in)."""
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Werror", "-DARIA_HIP_USE_REFERENCE_HEADERS", "-I" + REF_INC,
                           "-I" + os.path.join(ROOT, "tests", "cpp", "eigen_standin"), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), "-c", os.path.join(PKG, "host", "src", "HipSensorFusion.cpp"),
                           "-o", str(tmp_path / "HipSensorFusion.o")])
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "aria_hip/HipSensorFusion.hpp"\n'
                     "aria::interfaces::SensorFusionPtr make() { return std::make_unique<aria::adapters::hip::HipSensorFusion>(); }\n"
                     "static_assert(std::is_same<decltype(std::declval<aria::interfaces::ISensorFusion&>().getVelocity()), "
                     "Eigen::Vector3d>::value, \"the real port\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-Werror", "-DARIA_HIP_USE_REFERENCE_HEADERS", "-I" + REF_INC,
                           "-I" + os.path.join(ROOT, "tests", "cpp", "eigen_standin"), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), "-c", str(probe), "-o", str(tmp_path / "probe.o")])


def _asl_imu(L, root, cap=4096, image_cap=256):
    samples, ranges, n_img = np.zeros((cap, 7)), np.zeros((image_cap, 2), np.int32), C.c_int()
    n = L.aria_asl_imu(str(root).encode(), samples.ctypes.data, cap, ranges.ctypes.data, image_cap, C.byref(n_img))
    return n, samples[:max(n, 0)], ranges[:n_img.value]


def write_imu_csv(root, rows, shuffle=True):
    """rows: (t_ns, gyro xyz, accel xyz) as EuRoC stores them; written out of order, with a comment and a short row."""
    d = os.path.join(str(root), "mav0", "imu0")
    os.makedirs(d, exist_ok=True)
    lines = ["%d,%r,%r,%r,%r,%r,%r" % ((int(r[0]),) + tuple(float(x) for x in r[1:])) for r in rows]
    if shuffle:
        lines = lines[5:] + lines[:5]
    with open(os.path.join(d, "data.csv"), "w") as f:
        f.write("#timestamp [ns],w_RS_S_x [rad s^-1],w_y,w_z,a_RS_S_x [m s^-2],a_y,a_z\n" + "\n".join(lines[:7]) +
                "\n# a comment\n123,1.0,2.0\n\n" + "\n".join(lines[7:]) + "\n")


def test_asl_sequence_reads_imu0_and_the_per_image_ranges(aria, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    aria.load_library()
    L = C.CDLL(os.path.join(PKG, "libaria_hip_adapters.so"))
    L.aria_asl_imu.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    t0 = 1403636579763555584
    cam = tmp_path / "mav0" / "cam0"
    (cam / "data").mkdir(parents=True)
    img_ts = [t0 + i * 50_000_000 for i in range(6)]
    (cam / "data.csv").write_text("#timestamp [ns],filename\n" + "\n".join("%d,%d.png" % (t, t) for t in img_ts) + "\n")
    # without imu0 the sequence still loads
    n, samples, ranges = _asl_imu(L, tmp_path)
    assert n == 0 and len(ranges) == 6 and not ranges.any()
    # 200 Hz from 12 ms before the first image to past the last one; one sample exactly on an image's time
    rng = np.random.default_rng(0)
    ts = [t0 - 12_000_000 + k * 5_000_000 for k in range(60)]
    ts[12] = img_ts[1]
    rows = [(t,) + tuple(rng.normal(size=6)) for t in ts]
    write_imu_csv(tmp_path, rows)
    n, samples, ranges = _asl_imu(L, tmp_path)
    assert n == 60 and np.all(np.diff(samples[:, 0]) >= 0)
    order = np.argsort([r[0] for r in rows], kind="stable")
    want = np.array([[rows[k][0] * 1e-9] + list(rows[k][4:7]) + list(rows[k][1:4]) for k in order])      # accel = columns 4-6
    assert np.array_equal(samples[:, 1:], want[:, 1:]) and np.abs(samples[:, 0] - want[:, 0]).max() < 1e-6
    # EuRoCReader::getNext: prev_image_time < t <= image_time, 0 before the first image; samples after the last image unused
    st = np.sort(np.array(ts, np.int64))
    for i, t in enumerate(img_ts):
        prev = img_ts[i - 1] if i else 0
        idx = np.nonzero((st > prev) & (st <= t))[0]
        assert (ranges[i, 0], ranges[i, 1]) == (idx[0], idx[-1] + 1), i
    assert ranges[0, 0] == 0 and ranges[1, 1] == 13 and ranges[-1, 1] < 60 and np.array_equal(ranges[1:, 0], ranges[:-1, 1])


# ---- the branches of the restatement on the case table (tests/fuse_cases.py) ------------------------------------------------
import collections   # noqa: E402
import types         # noqa: E402

import fuse_cases as FC   # noqa: E402


def _restatement_copy(*replacements):
    """A private copy of fusion_ref, compiled from its source with every (old, new) applied; `old` must occur exactly once."""
    from aria_slam_amd import fusion_ref
    src = open(fusion_ref.__file__).read()
    for old, new in replacements:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    mod = types.ModuleType("fusion_ref_copy")
    mod.__file__ = fusion_ref.__file__
    exec(compile(src, fusion_ref.__file__, "exec"), mod.__dict__)
    return mod


class _Census:
    """Counts the branches a copy of the restatement takes, by wrapping its functions (the restatement itself has no hook):
    visits[branch] with the names of fuse_cases.BRANCH_CASE; qfr = (branch, trace, lead of the winning diagonal entry over the
    runner-up) per quat_from_rot; logw = w per log_map."""

    def __init__(self):
        m = self.mod = _restatement_copy()
        self.visits, self.qfr, self.logw, self.turned = collections.Counter(), [], [], 0
        qfr, logm, expm, qaa, chol, add_imu = m.quat_from_rot, m.log_map, m.exp_map, m.quat_angle_axis, m.cholesky_lower, m.SensorFusion.add_imu

        def quat_from_rot(Rm):
            Rm = np.asarray(Rm)
            d = [Rm[0, 0], Rm[1, 1], Rm[2, 2]]
            tr = d[0] + d[1] + d[2]
            q = qfr(Rm)
            if tr > 0:
                branch, lead = "trace", None
            else:
                i = 1 if d[1] > d[0] else 0
                i = 2 if d[2] > d[i] else i
                branch, lead = "xyz"[i], d[i] - max(d[j] for j in range(3) if j != i)
                j, k = (i + 1) % 3, (i + 2) % 3
                assert q[1 + i] == Rm.dtype.type(0.5) * np.sqrt(d[i] - d[j] - d[k] + Rm.dtype.type(1))    # it is the branch taken
            self.visits["qfr_" + branch] += 1
            self.qfr.append((branch, tr, lead))
            return q

        def log_map(q):
            n = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
            self.visits["log_n_zero" if n == 0 else ("log_w_neg" if q[0] < 0 else "log_w_pos")] += 1
            self.logw.append(q[0])
            return logm(q)

        def quat_angle_axis(angle, v):
            self.turned += 1
            return qaa(angle, v)

        def exp_map(theta):
            before = self.turned
            out = expm(theta)
            self.visits["update_turns" if self.turned > before else "update_zero_angle"] += 1
            return out

        def cholesky_lower(S):
            L, ok = chol(S)
            if not ok:
                a = [k for k in range(len(S)) if L[k, k] == 0][0]          # pivots before the failing one are > 0
                self.visits["notpd_later_pivot" if a else ("notpd_zero_pivot" if S[0, 0] == 0 else "notpd_first_pivot")] += 1
            return L, ok

        def wrapped_add_imu(flt, t, accel, gyro):
            resume = flt.initialized and flt.last_imu_time < 0
            predicted, turned = flt.n_predicted, self.turned
            add_imu(flt, t, accel, gyro)
            if resume:
                assert flt.n_predicted == predicted
                self.visits["resume_skip"] += 1
            if flt.n_predicted > predicted:
                self.visits["predict_turns" if self.turned > turned else "predict_zero_angle"] += 1

        m.quat_from_rot, m.log_map, m.exp_map, m.quat_angle_axis, m.cholesky_lower = quat_from_rot, log_map, exp_map, quat_angle_axis, cholesky_lower
        m.SensorFusion.add_imu = wrapped_add_imu

    def run(self, flt, imu, end, vis):
        return self.mod.run_track(flt, imu, end, vis)


_census_cache = {}


def _case_census(name, dtype=np.float64):
    key = (name, np.dtype(dtype))
    if key not in _census_cache:
        c = _Census()
        tr = FC.track(name)
        c.states = c.run(FC.ref_filter(tr, dtype, mod=c.mod), tr.imu, tr.imu_end, tr.visual)
        _census_cache[key] = c
    return _census_cache[key]


def test_census_every_branch_is_visited_by_the_case_named_for_it():
    """The table as a whole visits every branch the device spells out, and BRANCH_CASE names the case for each."""
    total = collections.Counter()
    for name in FC.NAMES:
        c = _case_census(name)
        total.update(c.visits)
        print("%-10s %s" % (name, dict(sorted(c.visits.items()))))
    assert set(total) == set(FC.BRANCH_CASE)
    for branch, name in FC.BRANCH_CASE.items():
        assert _case_census(name).visits[branch] > 0, (branch, name)
    # the wrapped copy computes what the restatement computes
    want = FC.ref_runs("turn_z")[0]
    assert all(np.array_equal(_case_census("turn_z").states[k], want[k]) for k in want)
    # the figures of the turning track: 81 frames, one initialises; the trace branch 54 times, the z-largest 27 times, and
    # w < 0 in 47 of 80 innovations
    v = _case_census("turn_z").visits
    assert (v["qfr_trace"], v["qfr_z"], v["qfr_x"], v["qfr_y"]) == (54, 27, 0, 0)
    assert (v["log_w_neg"], v["log_w_pos"], v["log_n_zero"]) == (47, 33, 0) and v["predict_turns"] == 800
    for name, b in (("turn_x", "qfr_x"), ("turn_y", "qfr_y")):             # the same turn in the other two branches
        v = _case_census(name).visits
        assert (v["qfr_trace"], v[b], v["log_w_neg"]) == (54, 27, 47) and sum(v["qfr_" + a] for a in ("x", "y", "z")) == 27
    # ties: which branch each rotation takes (exact entries: in any precision), and that its five updates turn nothing
    branch = dict(ties_x="x", ties_y="y", ties_z="z", ties_xy="x", ties_yz="y", ties_zx="x", ties_111="x", ties_xny="x",
                  ties_ynz="y", ties_xnz="x", ties_111n="x")
    for name in FC.TIES:
        c = _case_census(name)
        assert c.visits["qfr_" + branch[name]] == 6 and c.visits["update_zero_angle"] == 5 and c.visits["update_turns"] == 0, name
        assert c.visits["log_n_zero"] + c.visits["log_w_pos"] + c.visits["log_w_neg"] == 5
    assert _case_census("ties_111").visits["log_n_zero"] == 5 and _case_census("ties_x").visits["log_n_zero"] == 5
    # notpd: the first frame's rejection is where the case says; zero_gyro: ten steps of angle 0; resume: one skip
    assert _case_census("notpd_a").visits["notpd_first_pivot"] >= 1 and _case_census("notpd_a").states["n_updates"][0] == 0
    assert _case_census("notpd_b").visits["notpd_later_pivot"] >= 1 and _case_census("notpd_b").states["n_updates"][0] == 0
    assert _case_census("notpd_c").visits["notpd_zero_pivot"] == 1 and _case_census("notpd_c").states["n_updates"][0] == 0
    assert _case_census("zero_gyro").visits["predict_zero_angle"] == 10
    assert _case_census("resume").visits["resume_skip"] == 1 and _case_census("resume").states["n_skipped"][0] == 1


def test_census_the_old_tracks_visit_none_of_the_new_branches():
    """What tests/test_gpu_fuse.py runs on the device stays near R = I: the trace branch, w > 0, both guards on the turning
    side, no rejected pivot, no resumed record. (Why tests/fuse_cases.py exists; checked so that the claim stays true.)"""
    import test_gpu_fuse as TG
    for name in TG.TRACKS:
        c = _Census()
        c.run(c.mod.SensorFusion(), *TG.make_track(name))
        assert set(c.visits) == FC.OLD_BRANCHES, (name, dict(c.visits))
        tr_min = min(float(t) for _b, t, _l in c.qfr)
        w_min = min(abs(float(w)) for w in c.logw)
        print("%-8s %s smallest trace %.3f smallest |w| %.5f" % (name, dict(c.visits), tr_min, w_min))
        assert tr_min > 2.9 and w_min > 0.99


def test_decision_margins_of_the_turning_tracks_and_exact_ties():
    """A different quat_from_rot branch or sign of w is not a rounding difference, so no decision may hang on rounding: the
    fp64 and the extended run take the same branch at every call, every trace is 1e-9 from 0, every winning diagonal entry
    leads by 1e-9, every |w| handed to log_map is above 1e-3. Measured: smallest |trace| 0.035, lead 1.5, |w| 0.9998."""
    for name in FC.TURNING:
        a, b = _case_census(name), _case_census(name, np.longdouble)
        assert [x[0] for x in a.qfr] == [x[0] for x in b.qfr] and len(a.qfr) == 81
        assert [w < 0 for w in a.logw] == [w < 0 for w in b.logw] and len(a.logw) == 80
        assert a.visits == b.visits
        for c in (a, b):
            tr_min = min(abs(float(t)) for _b, t, _l in c.qfr)
            lead = min(float(l) for _b, _t, l in c.qfr if l is not None)
            w_min = min(abs(float(w)) for w in c.logw)
            print("%-10s %-10s |trace| >= %.3g  lead >= %.3g  |w| >= %.5f" % (name, c.states["p"].dtype, tr_min, lead, w_min))
            assert tr_min >= 1e-9 and lead >= 1e-9 and w_min >= 1e-3
    for name in FC.TIES:
        for _t, Rm, _p, _a in FC.track(name).visual:
            assert np.array_equal(Rm, np.round(Rm)) and abs(np.linalg.det(Rm) - 1) < 1e-15 and np.array_equal(Rm @ Rm.T, np.eye(3))
        assert _case_census(name).visits == _case_census(name, np.longdouble).visits
    # every other decision of the table (skips, rejected pivots) falls the same way in both precisions
    for name in FC.NAMES:
        FC.measure_gap(name)


_SWAP = ("    q[1 + j] = (R[j, i] + R[i, j]) * s\n    q[1 + k] = (R[k, i] + R[i, k]) * s\n",
         "    a, b = (k, j) if i == %d else (j, k)\n    q[1 + a] = (R[j, i] + R[i, j]) * s\n    q[1 + b] = (R[k, i] + R[i, k]) * s\n")
_WSIGN = ("    q[0] = (R[k, j] - R[j, k]) * s\n", "    q[0] = ((R[j, k] - R[k, j]) if i == %d else (R[k, j] - R[j, k])) * s\n")
_GE1 = ("    if R[1, 1] > R[0, 0]:\n", "    if R[1, 1] >= R[0, 0]:\n")
_GE2 = ("    if R[2, 2] > R[i, i]:\n", "    if R[2, 2] >= R[i, i]:\n")
_GE0 = ("    if tr > 0:\n", "    if tr >= 0:\n")
MUTANTS = [   # (what is altered, (old, new), the case that must catch it)
    ("the off-diagonal sums of the x-largest branch swapped", (_SWAP[0], _SWAP[1] % 0), "turn_x"),
    ("the off-diagonal sums of the y-largest branch swapped", (_SWAP[0], _SWAP[1] % 1), "turn_y"),
    ("the off-diagonal sums of the z-largest branch swapped", (_SWAP[0], _SWAP[1] % 2), "turn_z"),
    ("the difference of the x-largest branch transposed", (_WSIGN[0], _WSIGN[1] % 0), "turn_x"),
    ("the difference of the y-largest branch transposed", (_WSIGN[0], _WSIGN[1] % 1), "turn_y"),
    ("the difference of the z-largest branch transposed", (_WSIGN[0], _WSIGN[1] % 2), "turn_z"),
    ("x against y: the later of equals", _GE1, "ties_xny"),
    ("y against z: the later of equals", _GE2, "ties_ynz"),
    ("x against z: the later of equals", _GE2, "ties_xnz"),
    ("trace 0 takes the trace branch", _GE0, "ties_111n"),
    ("log_map keeps the axis when w < 0", ("    if q[0] < 0:\n        n = -n\n", ""), "turn_z"),
    ("a failed first pivot goes on into the update",
     ("                if not s > 0:\n                    return L, False\n", "                if not s > 0:\n                    s = S.dtype.type(1)\n"), "notpd_a"),
    ("a failed later pivot goes on into the update",
     ("                if not s > 0:\n                    return L, False\n", "                if not s > 0:\n                    s = S.dtype.type(1)\n"), "notpd_b"),
    ("a pivot of exactly 0 goes on into the update",
     ("                if not s > 0:\n                    return L, False\n", "                if not s > 0:\n                    s = S.dtype.type(1)\n"), "notpd_c"),
    # (`not s >= 0` in place of `not s > 0` is no mistake anything can see: the zero pivot divides the column below it into
    # NaN or inf, and the next pivot fails instead. notpd_c pins that a zero pivot is rejected, not which test rejects it.)
    ("the prediction without its angle guard",
     ("        if angle > 1e-10:\n            self.orientation = ", "        if True:\n            self.orientation = "), "zero_gyro"),
    ("the update without its angle guard", ("    if angle < 1e-10:\n        return np.array([1, 0, 0, 0], dtype=theta.dtype)\n", ""), "ties_111"),
]


def _departure(name, mod):
    """(largest state difference, largest P difference relative to the true P, a counter differs) of a copy of the
    restatement against the restatement itself on a case, both in fp64; a NaN counts as infinitely far."""
    tr = FC.track(name)
    want, f64 = FC.ref_runs(name)[:2]
    flt = FC.ref_filter(tr, mod=mod)
    with np.errstate(all="ignore"):
        got = mod.run_track(flt, tr.imu, tr.imu_end, tr.visual)
        ds = max(float(np.nan_to_num(np.abs(got[k] - want[k]), nan=np.inf).max()) for k in FC.STATE_KEYS)
        dp = float(np.nan_to_num(np.abs(flt.P - f64.P), nan=np.inf).max() / np.abs(f64.P).max())
    return ds, dp, any(not np.array_equal(got[k], want[k]) for k in FC.COUNTERS)


@pytest.mark.parametrize("what,replacement,name", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_the_table_catches_an_altered_restatement(what, replacement, name):
    """Each mistake the device could make in a branch, made in a copy of the restatement (never in the kernel): the case
    named for the branch departs from the true restatement by 1000 times its allowance at least, or in a counter."""
    ds, dp, counter = _departure(name, _restatement_copy(replacement))
    allow_s, allow_p = FC.allowed(name)
    print("%s on %s: states %.3g (allowance %.3g)  P %.3g (allowance %.3g)  counter %s" % (what, name, ds, allow_s, dp, allow_p, counter))
    assert ds >= 1000 * allow_s or dp >= 1000 * allow_p or counter


def test_the_listed_ties_alone_would_not_catch_a_tie_rule_and_the_unaltered_copy_departs_by_nothing():
    """Why fuse_cases adds four rotations to the issue's seven: on the half turns about (1,1,0), (0,1,1), (1,0,1) and the
    120 degree turn about (1,1,1) every component that could lead is positive, so either side of the tie gives the same
    quaternion up to rounding, and a wrong tie rule stays inside the allowance."""
    for replacement, name in ((_GE1, "ties_xy"), (_GE2, "ties_yz"), (_GE2, "ties_zx"), (_GE0, "ties_111"), (_GE1, "ties_111")):
        ds, dp, counter = _departure(name, _restatement_copy(replacement))
        assert ds <= FC.allowed(name)[0] and dp <= FC.allowed(name)[1] and not counter, (name, ds, dp)
    for name in ("turn_x", "ties_xny", "notpd_b", "zero_gyro"):
        assert _departure(name, _restatement_copy()) == (0.0, 0.0, False)


def test_preintegration_cases_reach_the_zero_angle_branch_and_a_negative_w():
    from aria_slam_amd import fusion_ref as R
    a, b = FC.preint_refs("zero_angle")
    for r in (a, b):
        assert np.array_equal(r["delta_q"][:10], np.tile([1.0, 0, 0, 0], (10, 1))) and (r["n_used"] == 19).all()
        assert (np.abs(r["delta_q"][10:, 1:]).max(axis=1) > 1e-3).all()
        assert (r["cov"][:10, 6, 6] > 0).all() and (r["cov"][:10, 7, 7] > 0).all() and (r["cov"][:10, 8, 8] > 0).all()
    a, b = FC.preint_refs("full_turn")
    assert a["delta_q"][0, 0] < -0.9 and b["delta_q"][0, 0] < -0.9 and a["n_used"][0] == 799       # a whole turn: w ends near -1
    imu = FC.preint_case("full_turn")[0]
    half = R.preintegrate(imu, [0], [400], FC.PREINT_BIAS)
    assert abs(half["delta_q"][0, 0]) < 0.1                                                            # ... and crosses 0 on the way
    assert FC.preint_refs("epoch")[0]["n_used"][0] == 799
    # without its angle guard the preintegrator divides 0 by 0 on the first kind, and on that kind only
    imu, begin, end, bias = FC.preint_case("zero_angle")
    mod = _restatement_copy(("        if angle > 1e-10:\n            self.delta_q = quat_mul(", "        if True:\n            self.delta_q = quat_mul("))
    with np.errstate(all="ignore"):
        got = mod.preintegrate(imu, begin, end, bias)
    assert np.isnan(got["delta_q"][:10]).all() and np.array_equal(got["delta_q"][10:], FC.preint_refs("zero_angle")[0]["delta_q"][10:])
