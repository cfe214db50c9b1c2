"""The fusion kernels (aria_slam_amd/csrc/imu_fusion.hip) on the branches that tests/test_gpu_fuse.py never reaches: the three
largest-diagonal blocks of quat_from_rot and the order of their comparisons, w < 0 and n == 0 in the log map, a rejected
Cholesky pivot (the first, a later one, one of exactly 0), a step and an update of angle 0, a record resumed with
last_imu_time < 0, gravity along x and y, timestamps of EuRoC's size, and the same guard in k_imu_preintegrate.

The cases are tests/fuse_cases.py's; tests/test_fuse_host.py shows with the restatement alone that they visit those branches,
that no decision on them hangs on rounding, and that each catches the mistake it is there for. The tolerance is the rule of
test_gpu_fuse.py, unchanged: the device against fusion_ref in np.longdouble at ten times the case's CPU-measured fp64 gap
(fuse_cases.GAP, from tools/fuse_gap.py; scene1's row where a case measures less). Every figure is printed as a share of its
allowance; the largest per case is recorded in DESIGN.md section 14."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_cases as FC   # noqa: E402
from test_gpu_fuse import ARIA_E_INVALID, _launch, _state_diff, fu, torch_cuda   # noqa: E402, F401

pytestmark = pytest.mark.gpu


def _bits_equal(rec, other, fields):
    return all(rec[k].tobytes() == other[k].tobytes() for k in fields)


@pytest.mark.parametrize("name", FC.NAMES)
def test_every_case_matches_the_extended_restatement(aria, fu, name):
    from aria_slam_amd import fusion as FU
    tr = FC.track(name)
    _s64, _f64, sld, fld = FC.ref_runs(name)
    allow_s, allow_p = FC.allowed(name)
    filt = FC.record(tr)
    st = fu.run(tr.imu, tr.imu_end, tr.visual, filt)
    assert st["valid"].all() and np.isfinite(st["p"]).all() and np.isfinite(st["q"]).all() and np.isfinite(filt[0]["P"]).all()
    for k in FC.COUNTERS:
        assert np.array_equal(st[k], sld[k]), k
    assert np.array_equal(st["t"], np.array([v[0] for v in tr.visual]))
    ds = _state_diff(st, sld)
    pmax = float(np.abs(fld.P).max())
    dd = float(np.abs(st["P_diag"].astype(np.longdouble) - sld["P_diag"]).max() / max(float(np.abs(sld["P_diag"]).max()), 1e-300))
    P = filt[0]["P"].reshape(15, 15)
    dp = float(np.abs(P.astype(np.longdouble) - fld.P).max() / pmax)
    fin = FU.filter_from_ref(fld)[0]
    dfin = max(float(np.abs(filt[0][k].astype(np.longdouble) - getattr(fld, a)).max()) for k, a in zip(FC.STATE_KEYS, FC.FILTER_ATTRS))
    print("%s: share of the allowance: states %.3f  final state %.3f  P_diag %.3f  final P %.3f  (allowed %.2e, %.2e)" %
          (name, ds / allow_s, dfin / allow_s, dd / allow_p, dp / allow_p, allow_s, allow_p))
    assert ds <= allow_s and dfin <= allow_s
    assert dd <= allow_p and dp <= allow_p
    assert filt[0]["last_imu_time"] == float(fld.last_imu_time) and filt[0]["last_visual_time"] == float(fld.last_visual_time)
    assert filt[0]["initialized"] == int(fld.initialized) == 1
    assert _bits_equal(filt[0], fin, ("gravity", "accel_noise", "gyro_noise", "accel_bias_walk", "gyro_bias_walk", "pos_noise", "rot_noise"))
    assert np.array_equal(P, P.T)
    if np.linalg.eigvalsh(np.asarray(fld.P, np.float64)).min() > 0:
        assert np.linalg.eigvalsh(P).min() > 0
    else:
        assert name in FC.NOTPD


@pytest.mark.parametrize("name", list(FC.NOTPD))
def test_a_rejected_pivot_leaves_state_and_covariance_alone(aria, fu, name):
    """The first frame of a notpd track, alone: no sample, one measurement the Cholesky rejects. No update is counted,
    last_visual_time moves, and the state and all of P keep the bits of the record that went in."""
    tr = FC.track(name)
    assert tr.imu_end[0] == 0 and tr.visual[0][3] == 1
    before = FC.record(tr)
    filt = before.copy()
    st = fu.run(tr.imu[:0], tr.imu_end[:1], tr.visual[:1], filt)
    assert st["valid"][0] == 1 and st["n_updates"][0] == 0 and st["n_predicted"][0] == 0 and st["initialized"][0] == 1
    assert filt[0]["last_visual_time"] == tr.visual[0][0] != before[0]["last_visual_time"]
    assert filt[0]["last_imu_time"] == before[0]["last_imu_time"]
    assert _bits_equal(filt[0], before[0], ("p", "v", "q", "ba", "bg", "P"))
    assert _bits_equal(st[0], before[0], ("p", "v", "q", "ba", "bg"))
    assert st[0]["P_diag"].tobytes() == np.diag(before[0]["P"].reshape(15, 15)).copy().tobytes()
    # the whole track: the frames after it run on (samples in between), and the first frame's record is what they start from
    whole = before.copy()
    sw = fu.run(tr.imu, tr.imu_end, tr.visual, whole)
    assert sw[:1].tobytes() == st.tobytes() and sw["n_predicted"][1:].sum() == len(tr.imu)


def test_a_step_of_angle_zero_keeps_the_orientation_bits(aria, fu):
    tr = FC.track("zero_gyro")
    assert not tr.imu[:int(tr.imu_end[1]), 4:7].any() and tr.visual[1][3] == 0
    filt = FC.record(tr)
    st = fu.run(tr.imu, tr.imu_end, tr.visual, filt)
    assert st["n_predicted"][1] == 10 and st["n_updates"][1] == 0
    assert st["q"][1].tobytes() == st["q"][0].tobytes() and not st["bg"][1].any()
    assert st["p"][1].tobytes() != st["p"][0].tobytes() and st["P_diag"][1].tobytes() != st["P_diag"][0].tobytes()   # it did predict
    assert st["q"][2].tobytes() != st["q"][1].tobytes()


def test_a_resumed_record_spends_its_first_sample_on_the_time(aria, fu):
    tr = FC.track("resume")
    before = FC.record(tr)
    assert before[0]["initialized"] == 1 and before[0]["last_imu_time"] == -1 and tr.imu_end[0] == 1 and tr.visual[0][3] == 0
    filt = before.copy()
    st = fu.run(tr.imu[:1], tr.imu_end[:1], tr.visual[:1], filt)
    assert (st["n_skipped"][0], st["n_predicted"][0], st["n_ignored"][0], st["n_updates"][0]) == (1, 0, 0, 0)
    assert filt[0]["last_imu_time"] == tr.imu[0, 0] and filt[0]["last_visual_time"] == before[0]["last_visual_time"]
    assert _bits_equal(filt[0], before[0], ("p", "v", "q", "ba", "bg", "P"))
    assert _bits_equal(st[0], before[0], ("p", "v", "q", "ba", "bg"))
    whole = before.copy()
    sw = fu.run(tr.imu, tr.imu_end, tr.visual, whole)
    assert sw[:1].tobytes() == st.tobytes() and sw["n_skipped"].sum() == 1 and sw["n_predicted"].sum() == len(tr.imu) - 1


def test_one_wave_four_different_paths(aria, fu, torch_cuda):
    """Eight tracks in two waves. Rows 0..3 of the first hold a rejected later pivot, a track that never starts, the x-largest
    turn and an exact tie; the second holds the y-largest turn, an invalid track, the epoch timestamps and the zero-angle
    steps. Every valid track has the bits of its run alone, the invalid one is flagged once, zeroed and its filter left
    alone; the same with the order reversed."""
    from aria_slam_amd import fusion as FU
    torch = torch_cuda
    z = FC.track("zero_gyro")
    never = (z.imu, z.imu_end, [v[:3] + (0,) for v in z.visual])
    t = FC.track("turn_z")
    bad_imu = t.imu[:int(t.imu_end[19])].copy()
    bad_imu[57, 5] = np.nan
    invalid = (bad_imu, t.imu_end[:20], t.visual[:20])
    named = [(n, FC.track(n)[:3], FC.record(FC.track(n))) for n in ("notpd_b", "turn_x", "ties_xy", "turn_y", "turn_epoch", "zero_gyro")]
    marked = FU.new_filter(1)
    marked["p"][0] = (1.0, 2.0, 3.0)
    entries = [named[0], ("never", never, FU.new_filter(1)), named[1], named[2], named[3], ("invalid", invalid, marked), named[4], named[5]]
    alone = {}
    for name, tr, rec in entries:
        if name != "invalid":
            one = rec.copy()
            alone[name] = (fu.run(tr[0], tr[1], tr[2], one), one)
    assert alone["never"][1][0]["initialized"] == 0 and alone["never"][0]["n_ignored"].sum() == len(z.imu)
    assert alone["never"][1].tobytes() == FU.new_filter(1).tobytes()
    for order in (entries, entries[::-1]):
        filt = np.concatenate([e[2] for e in order])
        f, s, status, fo = _launch(torch, fu, filt, [e[1] for e in order])
        assert status == ARIA_E_INVALID and fu.status() == 0            # flagged, once
        for k, (name, _tr, rec) in enumerate(order):
            got = s[fo[k]:fo[k + 1]]
            if name == "invalid":
                assert f[k:k + 1].tobytes() == rec.tobytes() and len(got) == 20
                assert not got["valid"].any() and not got.tobytes().strip(b"\0")
            else:
                assert got["valid"].all(), name
                assert got.tobytes() == alone[name][0].tobytes(), name
                assert f[k:k + 1].tobytes() == alone[name][1].tobytes(), name


@pytest.mark.parametrize("kind", FC.PREINT_KINDS)
def test_preintegration_zero_angle_full_turn_and_epoch(aria, kind):
    imu, begin, end, bias = FC.preint_case(kind)
    ref = FC.preint_refs(kind)[1]
    allow_s, allow_c = FC.allowed_preint(kind)
    pre = aria.HipImuPreintegrator()
    out = pre.preintegrate(imu, begin, end, bias)
    pre.close()
    assert out["valid"].all() and np.array_equal(out["n_used"], ref["n_used"])
    ds = max(float(np.abs(out[k].astype(np.longdouble) - ref[k]).max()) for k in ("delta_p", "delta_v", "delta_q", "dt_sum"))
    cov = out["cov"].reshape(-1, 9, 9)
    dc = float(np.abs(cov.astype(np.longdouble) - ref["cov"]).max()) / float(np.abs(ref["cov"]).max())
    print("preintegration %s: share of the allowance: deltas %.3f  covariance %.3f  (allowed %.2e, %.2e)" %
          (kind, ds / allow_s, dc / allow_c, allow_s, allow_c))
    assert ds <= allow_s and dc <= allow_c
    if kind == "zero_angle":
        # the gyro samples equal the bias: delta_q keeps (1, 0, 0, 0) to the bit while the orientation block still grows
        assert out["delta_q"][:10].tobytes() == np.tile([1.0, 0.0, 0.0, 0.0], (10, 1)).tobytes()
        assert (cov[:10, [6, 7, 8], [6, 7, 8]] > 0).all() and (np.abs(out["delta_q"][10:, 1:]).max(axis=1) > 1e-3).all()
    elif kind == "full_turn":
        assert out["delta_q"][0, 0] < -0.9 and out["n_used"][0] == 799
