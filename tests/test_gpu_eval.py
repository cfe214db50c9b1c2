"""Trajectory evaluation on the device (include/aria_orb_hip.h, "trajectory evaluation") against its NumPy restatement
(aria_slam_amd/eval_ref.py), which is the definition.

Tolerance is measured, not chosen (the convention of tests/test_gpu_fuse.py). The yardstick is the restatement in np.longdouble.
For every named track, GAP is the largest difference between its np.float64 and its np.longdouble run: the metric fields, t
and the per-pose errors absolute in metres; R and the scale absolute; the singular values relative. It is floored at one unit
in the last place of fp64 at the magnitude involved (eval_ref.result_gap). The device gets 10 x GAP against the extended run:
one decade for a different summation tree (strided lanes, a butterfly and four waves instead of index order) and different
sin, acos and sqrt. Nothing is compared with the device's own output except where bits must be identical.

GAP as measured on the CPU (tools/eval_gap.py prints this table; sim3 / se3):

    track      metres               R, scale             sigma (relative)   sigma2 / sigma1
    walk       1.61e-14 / 3.01e-14  1.88e-15 / 1.88e-15  4.59e-15           8.9e-02
    circle     1.18e-14 / 1.07e-14  6.79e-16 / 6.79e-16  9.28e-16           1.0e+00   two nearly equal singular values
    long       9.10e-14 / 1.26e-13  2.28e-15 / 1.91e-15  1.00e-14           2.9e-01   65 536 poses
    masked     5.71e-15 / 6.47e-15  5.25e-16 / 4.27e-16  5.49e-16           4.6e-01   30 % of the poses masked
    short      5.72e-16 / 1.08e-15  3.16e-16 / 3.16e-16  4.61e-16           1.9e-01   12 poses, delta 10
    corridor   6.32e-14 / 5.38e-14  9.67e-16 / 6.71e-16  1.95e-15           1.2e-05   what the SVD of C itself buys
    sampler    5.17e-16 (all fields, absolute)

What the device showed against the extended run on an MI355X is printed by the tests and recorded in DESIGN.md section 15."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")

# (metres, R / scale, sigma relative) per (track, mode): the table above
GAP = {
    ("walk", "sim3"): (1.61e-14, 1.88e-15, 4.59e-15), ("walk", "se3"): (3.01e-14, 1.88e-15, 4.59e-15),
    ("circle", "sim3"): (1.18e-14, 6.79e-16, 9.28e-16), ("circle", "se3"): (1.07e-14, 6.79e-16, 9.28e-16),
    ("long", "sim3"): (9.10e-14, 2.28e-15, 1.00e-14), ("long", "se3"): (1.26e-13, 1.91e-15, 1.00e-14),
    ("masked", "sim3"): (5.71e-15, 5.25e-16, 5.49e-16), ("masked", "se3"): (6.47e-15, 4.27e-16, 5.49e-16),
    ("short", "sim3"): (5.72e-16, 3.16e-16, 4.61e-16), ("short", "se3"): (1.08e-15, 3.16e-16, 4.61e-16),
    ("corridor", "sim3"): (6.32e-14, 9.67e-16, 1.95e-15), ("corridor", "se3"): (5.38e-14, 6.71e-16, 1.95e-15),
}
GAP_SAMPLER = 5.17e-16
MARGIN = 10
INT_FIELDS = ("n_poses", "n_used", "n_rpe_pairs", "align_valid", "valid")
METRE_FIELDS = ("ate_raw", "rpe_raw", "ate_rmse", "ate_mean", "ate_max", "rpe_aligned")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ev(aria):
    o = aria.HipTrajectoryEvaluator()
    yield o
    o.close()


def _ld(x):
    return np.asarray(x, np.longdouble)


def _diffs(rec, err, hi):
    """(metres, R / scale, sigma relative) of a device record and its per-pose errors against an extended evaluate()."""
    m = max([abs(_ld(rec[k]) - hi[k]) for k in METRE_FIELDS] + [np.abs(_ld(rec["t"]) - hi["t"]).max(),
                                                                 np.abs(_ld(err) - hi["pose_err"]).max()])
    r = max(np.abs(_ld(rec["R"]).reshape(3, 3) - hi["R"]).max(), abs(_ld(rec["scale"]) - hi["scale"]))
    s = (np.abs(_ld(rec["sigma"]) - hi["sigma"]) / hi["sigma"]).max()
    return float(m), float(r), float(s)


# ---- the device against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sim3", "se3"])
@pytest.mark.parametrize("name", ["walk", "circle", "long", "masked", "short", "corridor"])
def test_device_matches_the_restatement(aria, ev, name, mode):
    from aria_slam_amd import eval_ref as R
    e, g, mask, delta = R.named_track(name)
    hi = R.evaluate(e, g, R.ALIGN_NAMES[mode], delta, mask, np.longdouble)
    res, errs = ev.evaluate_batch([e], [g], masks=None if mask is None else [mask], align=mode, rpe_delta=delta, pose_errors=True)
    rec = res[0]
    for k in INT_FIELDS:
        assert int(rec[k]) == int(hi[k]), k
    assert rec["align_valid"] == 1 and rec["n_used"] == (len(e) if mask is None else int((mask != 0).sum()))
    m, r, s = _diffs(rec, errs[0], hi)
    gm, gr, gs = GAP[(name, mode)]
    print("eval %-8s %-4s device vs extended: metres %.2e (GAP %.2e) R/scale %.2e (GAP %.2e) sigma %.2e (GAP %.2e)"
          % (name, mode, m, gm, r, gr, s, gs))
    assert m <= MARGIN * gm and r <= MARGIN * gr and s <= MARGIN * gs
    if mode == "se3":
        assert rec["scale"] == 1.0
    if mask is not None:
        assert (errs[0][mask == 0] == -1).all() and (errs[0][mask != 0] >= 0).all()


def test_mode_none_is_the_reference_and_the_host_forms_agree(aria, ev):
    """Mode none: the aligned figures are computeATE / computeRPE again. Pose rows (n, 4, 4), (n, 12) and packed xyz read the
    same positions: the same bits."""
    from aria_slam_amd import eval_ref as R
    e, g, _, delta = R.named_track("walk")
    hi = R.evaluate(e, g, R.ALIGN_NONE, delta, None, np.longdouble)
    res, errs = ev.evaluate_batch([e], [g], align="none", pose_errors=True)
    m, r, s = _diffs(res[0], errs[0], hi)
    print("eval walk none device vs extended: metres %.2e R/scale %.2e sigma %.2e" % (m, r, s))
    gm, _gr, gs = GAP[("walk", "sim3")]
    assert m <= MARGIN * gm and r == 0 and s <= MARGIN * gs
    assert res[0]["ate_rmse"] == res[0]["ate_raw"] and res[0]["rpe_aligned"] == res[0]["rpe_raw"]
    T = np.tile(np.eye(4), (len(e), 1, 1))
    T[:, :3, 3] = e
    T[:, :3, :3] = np.random.default_rng(0).normal(size=(len(e), 3, 3))     # the rotation block is not read
    sim = ev.evaluate_batch([e], [g])
    assert ev.evaluate_batch([T], [g]).tobytes() == sim.tobytes()
    assert ev.evaluate_batch([T[:, :3, :].reshape(-1, 12)], [g]).tobytes() == sim.tobytes()
    from aria_slam_amd import evaluate as EV
    assert ev.evaluate_batch([e], EV.truth_from_positions(g), shared_truth=True).tobytes() == sim.tobytes()


def test_sampler_matches_the_restatement(aria, ev):
    from aria_slam_amd import eval_ref as R
    gt, q = R.sampler_case()
    hi, hv = R.sample_ground_truth(gt, q, np.longdouble)
    out, valid = ev.sample_ground_truth(gt, q)
    flat = out.view(np.float64).reshape(-1, 17)
    assert valid.all() and hv.all()
    d = float(np.abs(_ld(flat) - hi).max())
    print("eval sampler device vs extended: %.2e (GAP %.2e) over %d queries, %d rows" % (d, GAP_SAMPLER, len(q), len(gt)))
    assert d <= MARGIN * GAP_SAMPLER
    assert np.array_equal(flat[:, 0][2:-2], q[2:-2])                       # an interpolated sample carries the query's time
    # the clamps copy rows, bit for bit; an exact hit is its row, bit for bit (alpha = 1)
    assert np.array_equal(flat[0], gt[0]) and np.array_equal(flat[1], gt[0])
    assert np.array_equal(flat[-1], gt[-1]) and np.array_equal(flat[-2], gt[-1])
    assert np.array_equal(flat[-5], gt[1]) and np.array_equal(flat[-4], gt[777]) and np.array_equal(flat[-3], gt[35999])
    # the d < 0 branch and the near-parallel branch, on rows that hit them
    rows = np.zeros((3, 17))
    rows[:, 0] = [1.0, 2.0, 3.0]
    c, s = np.cos(0.5), np.sin(0.5)
    rows[:, 4:8] = [[0, 1, 0, 0], [-c, -s, 0, 0], [-c, -s, 0, 0]]
    hi2, _ = R.sample_ground_truth(rows, [1.5, 2.25], np.longdouble)
    out2, v2 = ev.sample_ground_truth(rows, [1.5, 2.25])
    assert v2.all() and float(np.abs(_ld(out2.view(np.float64).reshape(-1, 17)) - hi2).max()) <= MARGIN * GAP_SAMPLER
    assert out2["q"][0][0] > 0 and out2["q"][0][1] > 0                      # the far end was negated: towards (c, s, 0, 0)


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda")


def _launch(torch, ev, ests, truths, masks=None, kind=None, off=None, shared=None, mode="sim3", delta=10, n_total=None,
            n_truth=None, n_traj=None, want_err=True):
    """Raw aria_eval_batch_device over concatenated xyz trajectories; everything can be overridden. Returns (results, errors
    or None, status)."""
    from aria_slam_amd import _lib
    from aria_slam_amd import evaluate as EV
    kind = _lib.EVAL_EST_XYZ if kind is None else kind
    alle = np.concatenate([np.asarray(e, np.float64).reshape(-1, 3) for e in ests] + [np.zeros((1, 3))])
    NP = len(alle) - 1
    o = np.concatenate([[0], np.cumsum([len(e) for e in ests])]).astype(np.int32) if off is None else np.asarray(off, np.int32)
    allt = EV.truth_from_positions(shared) if shared is not None else \
        np.concatenate([EV.truth_from_positions(t) for t in truths] + [np.zeros(1, _lib.EVAL_TRUTH_DTYPE)])
    NT = len(allt) - (0 if shared is not None else 1)
    B = len(o) - 1 if n_traj is None else n_traj
    de, do, dt = _dev(torch, alle), _dev(torch, o), _dev(torch, allt)
    dm = None if masks is None else _dev(torch, np.concatenate([np.asarray(m, np.uint8) for m in masks] + [np.zeros(1, np.uint8)]))
    dres = torch.full((max(B, 1) * _lib.EVAL_RESULT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    derr = torch.full(((NP + 1) * 8,), 0xAB, dtype=torch.uint8, device="cuda") if want_err else None
    torch.cuda.synchronize()
    ev.evaluate_batch_device(de, kind, do, NP if n_total is None else n_total, B, dt, NT if n_truth is None else n_truth, dres,
                             truth_shared=shared is not None, d_mask=dm, align=mode, rpe_delta=delta, d_pose_err=derr)
    status = ev.status()
    res = np.frombuffer(dres.cpu().numpy().tobytes(), _lib.EVAL_RESULT_DTYPE)[:B].copy()
    err = np.frombuffer(derr.cpu().numpy().tobytes(), np.float64)[:NP].copy() if want_err else None
    return res, err, status


def _population(n_traj, seed, lo=3, hi=300):
    """n_traj random walks of different lengths, each with its own transform and noise."""
    rng = np.random.default_rng(seed)
    ests, truths = [], []
    for k in range(n_traj):
        n = int(rng.integers(lo, hi))
        g = np.cumsum(rng.normal(size=(n, 3)) * 0.1, axis=0) + rng.normal(size=3) * 5
        ests.append(g * rng.uniform(0.2, 3.0) + rng.normal(size=3) + 0.01 * rng.normal(size=(n, 3)))
        truths.append(g)
    return ests, truths


def test_bitwise_runs_position_neighbours_and_split(aria, ev, torch_cuda):
    from aria_slam_amd import eval_ref as R
    ests, truths = _population(1000, 1)
    e, g, _, _ = R.named_track("walk")
    ests[617], truths[617] = e, g
    a, ea, st = _launch(torch_cuda, ev, ests, truths)
    assert st == 0 and (a["valid"] == 1).all()
    b, eb, st = _launch(torch_cuda, ev, ests, truths)
    assert st == 0 and a.tobytes() == b.tobytes() and ea.tobytes() == eb.tobytes()          # run to run
    off = np.concatenate([[0], np.cumsum([len(x) for x in ests])])
    alone, e1, st = _launch(torch_cuda, ev, [e], [g])
    assert st == 0 and alone[0].tobytes() == a[617].tobytes() and e1.tobytes() == ea[off[617]:off[618]].tobytes()
    # other neighbours, another place
    ests2, truths2 = _population(1000, 2)
    ests2[3], truths2[3] = e, g
    c, ec, st = _launch(torch_cuda, ev, ests2, truths2)
    off2 = np.concatenate([[0], np.cumsum([len(x) for x in ests2])])
    assert st == 0 and c[3].tobytes() == a[617].tobytes() and ec[off2[3]:off2[4]].tobytes() == e1.tobytes()
    # the batch split into two calls
    p, ep, st1 = _launch(torch_cuda, ev, ests[:400], truths[:400])
    q, eq, st2 = _launch(torch_cuda, ev, ests[400:], truths[400:])
    assert st1 == st2 == 0 and p.tobytes() + q.tobytes() == a.tobytes() and ep.tobytes() + eq.tobytes() == ea.tobytes()
    # and the host-array form gives the same bits as the device form
    h, eh = ev.evaluate_batch(ests[:50], truths[:50], pose_errors=True)
    assert h.tobytes() == a[:50].tobytes() and np.concatenate(eh).tobytes() == ea[:off[50]].tobytes()


def test_a_call_larger_than_one_launch_is_split_without_a_trace(aria, ev, torch_cuda):
    """More than 32768 trajectories go out as several launches; the split must not show."""
    ests, truths = _population(40000, 3, lo=3, hi=24)
    a, ea, st = _launch(torch_cuda, ev, ests, truths, delta=4)
    assert st == 0 and (a["valid"] == 1).all() and (a["n_poses"] == [len(x) for x in ests]).all()
    p, ep, st1 = _launch(torch_cuda, ev, ests[:17001], truths[:17001], delta=4)
    q, eq, st2 = _launch(torch_cuda, ev, ests[17001:], truths[17001:], delta=4)
    assert st1 == st2 == 0 and p.tobytes() + q.tobytes() == a.tobytes() and ep.tobytes() + eq.tobytes() == ea.tobytes()
    from aria_slam_amd import eval_ref as R
    for k in (0, 32767, 32768, 39999):
        hi = R.evaluate(ests[k], truths[k], R.ALIGN_SIM3, 4, None, np.longdouble)
        assert int(a[k]["align_valid"]) == int(hi["align_valid"]) and int(a[k]["n_rpe_pairs"]) == hi["n_rpe_pairs"]
        assert abs(float(a[k]["ate_raw"] - hi["ate_raw"])) <= 1e-13


# ---- device-resident chains ------------------------------------------------------------------------------------------------------
def test_graph_poses_go_straight_into_the_evaluator(aria, ev, torch_cuda):
    """optimize_batch_device leaves poses and takes vertex offsets; both go into evaluate_batch_device as they are."""
    torch = torch_cuda
    from aria_slam_amd import _lib, graph_ref as G, eval_ref as R, posegraph as PG, evaluate as EV
    graphs, truths = [], []
    for seed, n in ((1, 120), (2, 60), (3, 200)):
        truth, init, odo, loops = G.circle_scene(seed, n=n)
        graphs.append((init, odo + loops, 0))
        truths.append(truth[:, :3, 3])
    rows = [PG.pack_poses(gr[0]) for gr in graphs]
    recs = [PG.pack_edges(gr[1]) for gr in graphs]
    voff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    eoff = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
    dp, dv, de, do = _dev(torch, np.concatenate(rows)), _dev(torch, voff), _dev(torch, np.concatenate(recs)), _dev(torch, eoff)
    df = _dev(torch, np.zeros(3, np.int32))
    dgres = torch.zeros(3 * _lib.GRAPH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dt = _dev(torch, EV.truth_from_positions(np.concatenate(truths)))
    dres = torch.zeros(3 * _lib.EVAL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    opt = aria.HipPoseGraphOptimizer(max_graphs=4, max_vertices=256, max_edges=512)
    ev2 = aria.HipTrajectoryEvaluator(stream=opt.stream, align="se3")              # one stream: no host synchronisation between
    torch.cuda.synchronize()
    opt.optimize_batch_device(dp, dv, de, do, df, 3, 10, dgres)
    ev2.evaluate_batch_device(dp, _lib.EVAL_EST_POSE12, dv, int(voff[-1]), 3, dt, int(voff[-1]), dres)
    assert ev2.status() == 0 and opt.status() == 0
    res = np.frombuffer(dres.cpu().numpy().tobytes(), _lib.EVAL_RESULT_DTYPE)
    poses = np.frombuffer(dp.cpu().numpy().tobytes(), np.float64).reshape(-1, 12)
    host = ev.evaluate_batch([poses[voff[k]:voff[k + 1]] for k in range(3)], truths, align="se3")
    assert host.tobytes() == res.tobytes()
    for k in range(3):
        est = poses[voff[k]:voff[k + 1]][:, [3, 7, 11]]
        hi = R.evaluate(est, truths[k], R.ALIGN_SE3, 10, None, np.longdouble)
        m, r, s = _diffs(res[k], hi["pose_err"], hi)      # the per-pose errors are not fetched here
        print("eval graph %d device vs extended: metres %.2e R %.2e sigma %.2e | ATE raw %.4f aligned %.4f"
              % (k, m, r, s, res[k]["ate_raw"], res[k]["ate_rmse"]))
        gm, gr_, gs = GAP[("circle", "se3")]             # the same shape (a circle of metres) and no more poses
        assert m <= MARGIN * gm and r <= MARGIN * gr_ and s <= MARGIN * gs
        d = est - truths[k]                               # computeATE with numpy: another path to the raw figure
        assert abs(float(res[k]["ate_raw"]) - float(np.sqrt((d * d).sum(1).mean()))) <= 1e-13
    ev2.close()
    opt.close()


def test_fused_states_go_straight_into_the_evaluator(aria, ev, torch_cuda):
    """run_batch_device leaves aria_fuse_state records; the frames before the filter is initialised are masked by the
    records' own flags."""
    torch = torch_cuda
    from aria_slam_amd import _lib, fusion as FU, fusion_ref as F, eval_ref as R, evaluate as EV
    tracks, truths = [], []
    for seed in (1, 2):
        sc = F.make_scene(seed, duration=6.0)
        vis = [(t, Rm, p, 0 if f < 5 else a) for f, (t, Rm, p, a) in enumerate(sc["visual"])]   # 5 frames before the first pose
        tracks.append((sc["imu"], sc["imu_end"], vis))
        truths.append(np.asarray(sc["truth_p"])[:len(vis)])
    fu = aria.HipSensorFusion()
    imus = [FU.pack_imu(t[0]) for t in tracks]
    viss = [FU.pack_visual(t[2]) for t in tracks]
    ioff = np.concatenate([[0], np.cumsum([len(x) for x in imus])]).astype(np.int32)
    foff = np.concatenate([[0], np.cumsum([len(x) for x in viss])]).astype(np.int32)
    NF = int(foff[-1])
    dflt, dimu, dio = _dev(torch, FU.new_filter(2)), _dev(torch, np.concatenate(imus)), _dev(torch, ioff)
    dend = _dev(torch, np.concatenate([np.asarray(t[1], np.int32) for t in tracks]))
    dvis, dfo = _dev(torch, np.concatenate(viss)), _dev(torch, foff)
    dst = torch.zeros(NF * _lib.FUSE_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dt = _dev(torch, EV.truth_from_positions(np.concatenate(truths)))
    dres = torch.zeros(2 * _lib.EVAL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    derr = torch.zeros(NF * 8, dtype=torch.uint8, device="cuda")
    ev2 = aria.HipTrajectoryEvaluator(stream=fu.stream)
    torch.cuda.synchronize()
    fu.run_batch_device(dflt, dimu, dio, int(ioff[-1]), dend, dvis, dfo, NF, 2, dst)
    ev2.evaluate_batch_device(dst, _lib.EVAL_EST_FUSE_STATE, dfo, NF, 2, dt, NF, dres, d_pose_err=derr)
    assert ev2.status() == 0 and fu.status() == 0
    res = np.frombuffer(dres.cpu().numpy().tobytes(), _lib.EVAL_RESULT_DTYPE)
    err = np.frombuffer(derr.cpu().numpy().tobytes(), np.float64)
    states = np.frombuffer(dst.cpu().numpy().tobytes(), _lib.FUSE_STATE_DTYPE)
    host, herr = ev.evaluate_batch([states[foff[k]:foff[k + 1]] for k in range(2)], truths, pose_errors=True)
    assert host.tobytes() == res.tobytes() and np.concatenate(herr).tobytes() == err.tobytes()
    for k in range(2):
        st = states[foff[k]:foff[k + 1]]
        mask = (st["initialized"] != 0) & (st["valid"] != 0)
        assert not mask[:5].any() and mask[5:].all() and res[k]["n_used"] == len(st) - 5 and res[k]["n_poses"] == len(st)
        assert (err[foff[k]:foff[k] + 5] == -1).all()
        hi = R.evaluate(st["p"], truths[k], R.ALIGN_SIM3, 10, mask, np.longdouble)
        lo = R.evaluate(st["p"], truths[k], R.ALIGN_SIM3, 10, mask, np.float64)
        gap = R.result_gap(lo, hi, np.concatenate([st["p"][mask], truths[k]]))       # this track's own GAP, measured the same way
        m, r, s = _diffs(res[k], err[foff[k]:foff[k + 1]], hi)
        print("eval fused %d device vs extended: metres %.2e (GAP %.2e) R/scale %.2e (GAP %.2e) sigma %.2e (GAP %.2e)"
              % (k, m, gap[0], r, gap[1], s, gap[2]))
        assert m <= MARGIN * gap[0] and r <= MARGIN * gap[1] and s <= MARGIN * gap[2]
    ev2.close()
    fu.close()


# ---- invalid input -------------------------------------------------------------------------------------------------------------
def test_invalid_trajectories_are_flagged_zeroed_and_do_not_disturb_neighbours(aria, ev, torch_cuda):
    torch = torch_cuda
    from aria_slam_amd import _lib
    ests, truths = _population(6, 5, lo=30, hi=60)
    good, egood, st = _launch(torch, ev, ests, truths)
    assert st == 0
    off = np.concatenate([[0], np.cumsum([len(x) for x in ests])]).astype(np.int32)
    zero = np.zeros(1, _lib.EVAL_RESULT_DTYPE)[0].tobytes()

    def others_equal(res, err, bad, skip=(), skip_err=()):
        for k in range(6):
            if k in skip:
                continue
            if k in bad:
                assert res[k].tobytes() == zero and res[k]["valid"] == 0, k
            else:
                assert res[k].tobytes() == good[k].tobytes(), k
                if k not in skip_err:
                    assert err[off[k]:off[k + 1]].tobytes() == egood[off[k]:off[k + 1]].tobytes(), k

    # a non-finite position of the estimate, of the truth
    for where in ("est", "truth"):
        e2, t2 = [x.copy() for x in ests], [x.copy() for x in truths]
        (e2 if where == "est" else t2)[2][7, 1] = np.nan if where == "est" else np.inf
        res, err, st = _launch(torch, ev, e2, t2)
        assert st == -1 and ev.status() == 0                                  # ARIA_E_INVALID, once
        others_equal(res, err, {2})
        assert not err[off[2]:off[3]].any()                                   # its per-pose errors are written as 0
    # ... but not where a mask takes the pose out
    e2 = [x.copy() for x in ests]
    e2[2][7, 1] = np.nan
    masks = [np.ones(len(x), np.uint8) for x in ests]
    masks[2][7] = 0
    res, err, st = _launch(torch, ev, e2, truths, masks=masks)
    assert st == 0 and res[2]["valid"] == 1 and res[2]["n_used"] == len(ests[2]) - 1 and err[off[2] + 7] == -1
    # offsets that decrease or leave the array: that trajectory only, nothing of it is written
    bad_off = off.copy()
    bad_off[4] = off[5] + 3                                                    # trajectory 4 runs backwards (3 is longer, and valid)
    res, err, st = _launch(torch, ev, ests, truths, off=bad_off)
    assert st == -1
    # 3 now ends inside 5's poses: both write the per-pose errors of those three poses, so only 5's others are compared
    others_equal(res, err, {4}, skip={3}, skip_err={5})
    assert res[3]["valid"] == 1 and res[3]["n_poses"] == off[5] + 3 - off[3]
    assert err[off[5] + 3:off[6]].tobytes() == egood[off[5] + 3:off[6]].tobytes()
    bad_off = off.copy()
    bad_off[6] = off[6] + 10                                                   # the last one leaves the array
    res, err, st = _launch(torch, ev, ests, truths, off=bad_off)
    assert st == -1
    others_equal(res, err, {5})
    assert err[off[5]:off[6]].tobytes() == b"\xab" * (8 * len(ests[5]))        # not written at all
    bad_off = off.copy()
    bad_off[0] = -2
    res, err, st = _launch(torch, ev, ests, truths, off=bad_off)
    assert st == -1
    others_equal(res, err, {0})
    # shared truth: only trajectories of its length are scored
    n3 = len(ests[3])
    res, err, st = _launch(torch, ev, ests, None, shared=truths[3])
    assert st == -1 and [int(v) for v in res["valid"]] == [1 if len(x) == n3 else 0 for x in ests]
    assert res[3].tobytes() == good[3].tobytes()
    same = [ests[3], ests[3] * 2.0, ests[3] + 1.0]
    res, err, st = _launch(torch, ev, same, None, shared=truths[3])
    assert st == 0 and res[0].tobytes() == good[3].tobytes() and (res["valid"] == 1).all()
    # delta < 1, an alignment mode that does not exist: every trajectory of the call
    for kw in (dict(delta=0), dict(delta=-3), dict(mode=7)):
        res, err, st = _launch(torch, ev, ests, truths, **kw)
        assert st == -1 and (res["valid"] == 0).all() and all(r.tobytes() == zero for r in res) and not err.any()
    # the evaluator is as good as new
    res, err, st = _launch(torch, ev, ests, truths)
    assert st == 0 and res.tobytes() == good.tobytes()


def test_invalid_ground_truth_tables(aria, ev):
    from aria_slam_amd import eval_ref as R
    gt = R.truth_rows(500, 3)
    q = np.linspace(gt[0, 0] - 0.1, gt[-1, 0] + 0.1, 77)
    good, valid = ev.sample_ground_truth(gt, q)
    assert valid.all() and ev.last_status == 0
    for what in ("decreasing", "nan", "empty"):
        bad = gt.copy()
        if what == "decreasing":
            bad[300, 0] = bad[298, 0]
        elif what == "nan":
            bad[499, 16] = np.nan
        else:
            bad = bad[:0]
        out, valid = ev.sample_ground_truth(bad, q, raise_on_error=False)
        assert ev.last_status == -1 and not valid.any() and not out.view(np.float64).any(), what
        with pytest.raises(aria.AriaError):
            ev.sample_ground_truth(bad, q)
    qq = q.copy()
    qq[5] = np.inf
    out, valid = ev.sample_ground_truth(gt, qq, raise_on_error=False)
    assert ev.last_status == -1 and valid.sum() == 76 and valid[5] == 0 and not out[5:6].view(np.float64).any()
    keep = np.arange(77) != 5
    assert out[keep].tobytes() == good[keep].tobytes()
    again, valid = ev.sample_ground_truth(gt, q)
    assert again.tobytes() == good.tobytes() and ev.status() == 0


def test_edges_no_trajectories_no_poses_degenerate(aria, ev, torch_cuda):
    from aria_slam_amd import eval_ref as R
    assert len(ev.evaluate_batch([], [])) == 0
    i = np.arange(12.0)
    g = np.stack([i, 0.5 * i, -0.25 * i], 1)
    cases = [np.zeros((0, 3)), np.stack([2.0 * i, 0 * i, 0 * i], 1), np.tile([1.0, 2.0, 3.0], (12, 1)), g[:2] + [0.5, 0, 0], g[:10] * 1.5]
    tr = [g[:0], g, g, g[:2], g[:10]]
    res, errs = ev.evaluate_batch(cases, tr, pose_errors=True)
    assert (res["valid"] == 1).all() and list(res["n_poses"]) == [0, 12, 12, 2, 10]
    assert res[0]["ate_raw"] == -1 and res[0]["rpe_raw"] == -1 and res[0]["align_valid"] == 0 and res[0]["ate_rmse"] == -1
    for k in (1, 2, 3):                                  # collinear, coincident, n = 2: raw fields filled, aligned fields -1
        lo = R.evaluate(cases[k], tr[k])
        assert res[k]["align_valid"] == 0 == lo["align_valid"] and res[k]["scale"] == -1 and (res[k]["R"] == -1).all()
        assert res[k]["ate_rmse"] == res[k]["ate_mean"] == res[k]["ate_max"] == res[k]["rpe_aligned"] == -1 and (errs[k] == -1).all()
        assert abs(res[k]["ate_raw"] - lo["ate_raw"]) <= 1e-14 and res[k]["ate_raw"] > 0
    assert res[1]["rpe_raw"] > 0 and res[3]["rpe_raw"] == -1
    assert res[4]["rpe_raw"] == -1 and res[4]["n_rpe_pairs"] == 0 and res[4]["ate_raw"] > 0        # n <= delta


# ---- C++ and the driver ------------------------------------------------------------------------------------------------------------
def _build_selftest():
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    exe = os.path.join(ROOT, "build", "eval_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "eval_selftest.cpp"), "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    return exe


def test_cpp_adapter_equals_the_python_class(aria, ev, tmp_path):
    """tests/cpp/eval_selftest.cpp drives HipTrajectoryEvaluator on a script; the Python class on the same arrays gives the
    same bits (the same library)."""
    from aria_slam_amd import eval_ref as R, _lib
    gt = R.truth_rows(400, 9)
    rng = np.random.default_rng(10)
    q = np.sort(rng.uniform(gt[0, 0] - 0.05, gt[-1, 0] + 0.05, 150))
    truth, valid = ev.sample_ground_truth(gt, q)
    est = truth["p"] * 0.5 + [1.0, -2.0, 0.5] + 0.01 * rng.normal(size=(150, 3))
    mask = (rng.uniform(size=150) > 0.2).astype(np.uint8)
    lines = ["mode 1", "delta 7"]
    lines += ["gt " + " ".join(repr(float(x)) for x in row) for row in gt]
    lines += ["q %r" % float(t) for t in q]
    lines += ["e %r %r %r %d" % (float(p[0]), float(p[1]), float(p[2]), int(m)) for p, m in zip(est, mask)]
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    out = subprocess.run([_build_selftest(), "run", str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    got_t = np.array([l.split()[1:] for l in out.stdout.splitlines() if l.startswith("truth ")], np.float64)
    assert got_t.shape == (150, 18) and got_t[:, 0].tolist() == valid.tolist()
    assert got_t[:, 1:].tobytes() == truth.tobytes()
    res, errs = ev.evaluate_batch([est], [truth], masks=[mask], align="se3", rpe_delta=7, pose_errors=True)
    r = res[0]
    got_r = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("result ")][0]
    want = np.concatenate([[r["ate_raw"], r["rpe_raw"], r["scale"]], r["R"], r["t"], r["sigma"],
                           [r["ate_rmse"], r["ate_mean"], r["ate_max"], r["rpe_aligned"]]])
    assert np.array(got_r[:22], np.float64).tobytes() == want.tobytes()
    assert [int(x) for x in got_r[22:]] == [int(r[k]) for k in INT_FIELDS] and r["valid"] == 1 and r["align_valid"] == 1
    got_e = np.array([l.split()[1] for l in out.stdout.splitlines() if l.startswith("err ")], np.float64)
    assert got_e.tobytes() == errs[0].tobytes()


def test_euroc_frontend_eval(aria, ev, tmp_path):
    """--eval FILE on a synthetic ASL tree with a ground-truth CSV: refused without --pose or without ground truth; the --pose
    file and the CSV are byte-identical with and without the flag; the figures are those of HipTrajectoryEvaluator on the
    written TUM trajectory. That file prints 9 decimals, so its positions are the driver's to 5e-10 m per coordinate: every
    figure in metres may differ by that times sqrt(3), times 1 / scale for the aligned ones through the estimate's spread --
    1e-7 covers a scale down to 0.01; the scale itself by 1e-9 relative to the trajectory's extent, 1e-6."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_eval_host import write_gt_csv
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    seq, t0 = _make_dataset(aria, str(tmp_path), 8, w=640, h=480)
    n = len(seq)
    exe = os.path.join(PKG, "euroc_frontend")
    p1, p2, c1, c2, e2 = (str(tmp_path / x) for x in ("p1.txt", "p2.txt", "c1.csv", "c2.csv", "eval.txt"))
    bad = subprocess.run([exe, str(tmp_path), "1000", "--eval", e2], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--eval needs --pose" in bad.stderr
    bad = subprocess.run([exe, str(tmp_path), "1000", "--pose", p2, "--eval", e2], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "no mav0/state_groundtruth_estimate0" in bad.stderr
    # ground truth at 200 Hz around the images, unsorted, with comment and short lines
    rng = np.random.default_rng(6)
    M = 10 * n + 30
    gts = [t0 - 60_000_000 + k * 5_000_000 + 1_234_567 for k in range(M)]
    pos = np.cumsum(rng.normal(size=(M, 3)) * 0.02, axis=0)
    quat = rng.normal(size=(M, 4)) * 0.05 + [1, 0, 0, 0]
    quat /= np.sqrt((quat * quat).sum(1))[:, None]
    rows = [(gts[k], np.concatenate([pos[k], quat[k], rng.normal(size=9) * 0.1])) for k in range(M)]
    order = list(range(5, M)) + list(range(5))
    write_gt_csv(os.path.join(str(tmp_path), "mav0", "state_groundtruth_estimate0", "data.csv"), [rows[k] for k in order],
                 ["# comment", "", "%d,1.0,2.0,3.0" % t0])
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", p1, "--csv", c1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run([exe, str(tmp_path), "1000", "--pose", p2, "--csv", c2, "--eval", e2, "--eval-align", "sim3", "--rpe-delta", "3"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(p1, "rb").read() == open(p2, "rb").read() and open(c1, "rb").read() == open(c2, "rb").read()
    keep = lambda text: [l for l in text.splitlines() if not l.startswith("frames ") and not l.startswith("Frame ") and
                         not l.startswith("pose updates")]
    extra = keep(run.stdout)[len(keep(plain.stdout)):]
    assert keep(run.stdout)[:len(keep(plain.stdout))] == keep(plain.stdout)        # what was printed before is still printed
    assert extra[0].startswith("eval pose: ") and extra[-3:-2] == ["Trajectory Error:"]
    line = open(e2).read().split()
    assert line[:4] == ["pose", "sim3", str(n), str(n)] and len(line) == 15
    got = np.array(line[4:], np.float64)
    assert extra[-2] == "  ATE (RMSE): %.4f m" % got[0] and extra[-1] == "  RPE (RMSE): %.4f m" % got[1]
    # the same figures from the Python class on the written trajectory
    tum = np.array([l.split() for l in open(p2).read().splitlines()], np.float64)
    img_t = np.array([(t0 + i * 50_000_000) * 1e-9 for i in range(n)])
    assert np.array_equal(tum[:, 0], img_t)
    gt = aria.load_ground_truth_csv(os.path.join(str(tmp_path), "mav0", "state_groundtruth_estimate0", "data.csv"))
    assert len(gt) == M
    truth, valid = ev.sample_ground_truth(gt, img_t)
    assert valid.all()
    r = ev.evaluate_batch([tum[:, 1:4]], [truth], align="sim3", rpe_delta=3)[0]
    want = np.concatenate([[r["ate_raw"], r["rpe_raw"], r["align_valid"], r["scale"], r["ate_rmse"], r["ate_mean"], r["ate_max"],
                            r["rpe_aligned"]], r["sigma"]])
    print("euroc_frontend --eval:", " ".join(line))
    print("against the Python class on the TUM file: %.2e" % np.abs(got - want).max())
    assert r["valid"] == 1 and r["n_used"] == n and got[2] == want[2]
    assert np.abs(got[[0, 1, 4, 5, 6, 7]] - want[[0, 1, 4, 5, 6, 7]]).max() <= 1e-7
    if r["align_valid"]:
        assert abs(got[3] - want[3]) <= 1e-6 * max(1.0, abs(want[3])) and np.abs(got[8:] - want[8:]).max() <= 1e-7
