"""The definition of frame-to-model tracking, aria_slam_amd/icp_ref.py, on the cases of tests/icp_cases.py: what it recovers,
what it loses, where min_pivot sits, what its configuration refuses, and the overflow bound of its integer system. No GPU.

Every figure asserted here was measured with the restatement itself and is printed before it is asserted; the bounds are
twice the measured worst over eight seeded perturbations (tests/icp_cases.py, MEASURED)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC   # noqa: E402
from aria_slam_amd import icp_ref as IR   # noqa: E402


@pytest.mark.parametrize("name", ("corner", "fused", "odd"))
def test_recovery_over_eight_perturbations(name):
    """Worst error over eight seeded true poses at the case's start distance: at most twice the measured worst; on corner and
    fused every seed ends nearer than it started."""
    worst, corr = [0.0, 0.0], []
    for truth in IC.perturbations(*IC.START[name]):
        f = IC.frame(name, truth=truth)
        t = IR.track(IC.config(f.K), f.D, f.M, f.N, f.Tm, f.T0)
        assert int(t.result["valid"]) == 1
        ang, dist = IC.pose_error(t.T, truth)
        ang0, dist0 = IC.pose_error(f.T0, truth)
        if name in ("corner", "fused"):
            assert ang < ang0 and dist < dist0, (ang, ang0, dist, dist0)
        worst = [max(worst[0], ang), max(worst[1], dist)]
        corr.append(int(t.result["n_corr"]))
    print("%s: worst %.3e rad %.3e m, %d..%d correspondences" % (name, worst[0], worst[1], min(corr), max(corr)))
    assert worst[0] <= 2 * IC.MEASURED[name][0] and worst[1] <= 2 * IC.MEASURED[name][1]
    assert worst[0] >= 0.5 * IC.MEASURED[name][0] and worst[1] >= 0.5 * IC.MEASURED[name][1]       # the table is the measurement


def test_every_case_is_valid_or_lost_as_the_table_says():
    for name in IC.SINGLES:
        t, trace = IC.ref(name)
        print(name, t.result, len(trace))
        assert int(t.result["valid"]) == (0 if name in IC.LOST else 1), name
        if name in IC.LOST:
            assert t.T.tobytes() == np.asarray(IC.frame(name).T0).tobytes() and int(t.result["iterations_run"]) == 1
    t, trace = IC.ref("plane")
    assert trace[0][2].count >= IC.config().min_corr and 0 < len(trace[0][2].pivots) < 6       # lost by the pivot rule
    t, trace = IC.ref("tiny")
    assert trace[0][2].count < IC.config().min_corr and trace[0][2].pivots == []                # lost by min_corr
    # converged: the guess is the truth. The fixed point of the nearest-pixel association is not the truth itself (rms 1.5 mm),
    # so a level does not stop in its first iteration, as it would with exact correspondences: measured, the levels stop by eps
    # after 3, 3 and 5 of their 4, 5 and 10 iterations, and the first step is 1.0e-3, thirty times below corner's.
    t, trace = IC.ref("converged")
    per_level = [[st.norm for lv, _, st in trace if lv == l] for l in range(3)]
    print("converged:", per_level)
    cfg = IC.config()
    assert all(0 < len(n) < its and n[-1] < cfg.eps for n, its in zip(per_level, cfg.iterations))
    assert per_level[0][0] < IC.ref("corner")[1][0][2].norm / 10


def test_fused_model_has_hits_without_a_normal():
    M, N = IC.fused_model()[:2]
    none = (M > 0) & ~N.any(axis=-1)
    print("fused: %d hits, %d of them without a normal" % (int((M > 0).sum()), int(none.sum())))
    assert none.sum() >= 10
    # and the reject of rule 3 meets them: some live pixel projects onto one
    f = IC.frame("fused")
    ok, J, r, ui, vi = IR.jacobians(IC.config(f.K), f.D, f.M, f.N, IR.relative(f.Tm, f.T0), IR.model_rotation(f.Tm), 1)
    assert (none[vi, ui] & ~ok).sum() >= 10 and not (none[vi, ui] & ok).any()


def test_min_pivot_is_the_geometric_mean_of_what_it_separates():
    """The least pivot / count over every accumulation of the valid cases, and the pivot / count at which `plane` is lost
    on each of its levels (the greatest of them): the default is their geometric mean, and both lie 10x away from it."""
    least = min(min(st.pivots) / st.count for name in IC.SINGLES if name not in IC.LOST for _, _, st in IC.ref(name)[1])
    f = IC.frame("plane")
    cfg = IC.config(f.K)
    lost_at = []
    for stride in cfg.strides:
        st = IR.solve(cfg, IR.system(cfg, f.D, f.M, f.N, IR.relative(f.Tm, f.T0), IR.model_rotation(f.Tm), stride))
        assert st.lost and st.count >= cfg.min_corr
        lost_at.append(abs(st.pivots[-1]) / st.count)
    greatest = max(lost_at)
    mean = math.sqrt(least * greatest)
    print("least valid pivot / count %.3e, greatest lost on plane %.3e, geometric mean %.3e, default %.3e" % (least, greatest, mean,
                                                                                                         cfg.min_pivot))
    assert cfg.min_pivot == IR.DEFAULTS["min_pivot"]
    assert least >= 10 * cfg.min_pivot and 10 * greatest <= cfg.min_pivot
    assert mean / 1.5 <= cfg.min_pivot <= mean * 1.5


BAD = (dict(K=(0.0, 1.0, 1.0, 1.0)), dict(K=(1.0, float("nan"), 1.0, 1.0)), dict(min_depth=0.0), dict(min_depth=2.0, max_depth=1.0),
       dict(max_depth=float("inf")), dict(dist_max=0.0), dict(dist_max=1.5), dict(dist_max=float("nan")), dict(reach=0.0),
       dict(reach=129.0), dict(min_corr=0), dict(min_corr=(1 << 24) + 1), dict(min_pivot=-1.0), dict(min_pivot=float("nan")),
       dict(eps=-1.0), dict(strides=(), iterations=()), dict(strides=(1,) * 5, iterations=(1,) * 5), dict(strides=(3,), iterations=(1,)),
       dict(strides=(32,), iterations=(1,)), dict(strides=(0,), iterations=(1,)), dict(strides=(1,), iterations=(65,)),
       dict(strides=(1,), iterations=(-1,)), dict(strides=(2, 1), iterations=(0, 0)), dict(strides=(2, 1), iterations=(1,)))
GOOD = (dict(), dict(dist_max=1.0, reach=128.0), dict(strides=(16, 1), iterations=(2, 0)), dict(strides=(1,), iterations=(64,)),
        dict(min_pivot=0.0, eps=0.0), dict(min_corr=1 << 24))


def test_configuration_validation():
    for kw in BAD:
        with pytest.raises(ValueError):
            IR.config(**kw)
    for kw in GOOD:
        IR.config(**kw)
    with pytest.raises(ValueError):
        IR.check_size(4097, 4096)
    IR.check_size(4096, 4096)


def test_bound_case_stays_inside_the_proven_bound():
    """`bound`: reach and dist_max at their maxima, depths that put |q| just inside reach and |e| just inside dist_max, normals
    just inside (n.n) <= 1.5: every accumulator is at most count x the per-term bound of the header's proof, and that bound
    times 2^24 terms is below 2^63."""
    cfg, D, M, N, trel, Rm = IC.bound_case()
    ok, J, r, _, _ = IR.jacobians(cfg, D, M, N, trel, Rm, 1)
    S = IR.system(cfg, D, M, N, trel, Rm, 1)
    count = int(S[28])
    print("bound: %d correspondences, max |J| %.3f of %.3f, max |r| %.4f of %.4f, max |A| %.4g of %.4g" %
          (count, np.abs(J).max(), IR.J_MAX, np.abs(r).max(), IR.R_MAX, float(np.abs(S[:21]).max()), count * IR.TERM_MAX[0]))
    assert count == int(ok.sum()) >= 8
    assert np.abs(J).max() <= IR.J_MAX and np.abs(r).max() <= IR.R_MAX
    assert np.abs(J).max() >= 0.5 * IR.J_MAX and np.abs(r).max() >= 0.4 * IR.R_MAX       # adversarial: near the bound
    assert all(abs(int(v)) <= count * IR.TERM_MAX[0] for v in S[:21])
    assert all(abs(int(v)) <= count * IR.TERM_MAX[1] for v in S[21:27]) and int(S[27]) <= count * IR.TERM_MAX[2]
    for term in IR.TERM_MAX:
        assert term * IR.MAX_PIXELS < 2.0 ** 63 and term * 64 * 256 < 2.0 ** 53      # int64 sums; exact fp64 sums of a wave


def test_far_map_first_accumulation_equals_corners_exactly():
    """Tm and T0 moved by 1 km: the 29 integers of the first accumulation are those of `corner`, the point of Trel; the pose
    that comes out differs from corner's, moved likewise, by the fp64 rounding of the composition only."""
    (tc, trace_c), (tf, trace_f) = IC.ref("corner"), IC.ref("far_map")
    assert (trace_c[0][1] == trace_f[0][1]).all() and trace_c[0][1][28] > 300
    assert all((a[1] == b[1]).all() for a, b in zip(trace_c, trace_f)) and tc.result.tobytes() == tf.result.tobytes()
    Rc, tcv = IC.split(tc.T)
    Rf, tfv = IC.split(tf.T)
    s = np.array(IC.FAR_SHIFT)
    dR, dt = np.abs(Rc - Rf).max(), np.abs((tcv - Rc @ s) - tfv).max()
    print("far_map: rotation differs by %.3e, translation by %.3e m" % (dR, dt))
    assert dR <= IC.FAR_MAP_BOUND and dt <= IC.FAR_MAP_BOUND


def test_masks_and_the_non_finite_rule():
    cfg = IC.config(IC.K)
    b = IC.batch(IC.FIVE, mask=[1, 0, 1, 1, 0])
    poses, recs, invalid = IC.expected(b, cfg)
    guard_p, guard_r = IC.guarded_outputs(5)
    assert not invalid
    for f in range(5):
        masked = f in (1, 4)
        assert (poses[f].tobytes() == guard_p[f].tobytes()) == masked and (recs[f:f + 1].tobytes() == guard_r[f:f + 1].tobytes()) == masked
    b = IC.batch(["corner", "corner", "converged"], nan_frame=1)
    poses, recs, invalid = IC.expected(b, cfg)
    assert invalid and recs[1:2].tobytes() == bytes(32) and poses[1].tobytes() == guard_p[1].tobytes()
    assert recs[0].tobytes() == IC.ref("corner")[0].result.tobytes() and poses[0].tobytes() == IC.ref("corner")[0].T.tobytes()


def test_levels():
    """(1,) x 1 is one debug_system + solve + advance; (16, 1) x (2, 0) runs two iterations on the coarsest stride only; the
    default runs at most 19."""
    f = IC.frame("corner")
    cfg = IC.config(f.K, **IC.LEVELS[0])
    t = IR.track(cfg, f.D, f.M, f.N, f.Tm, f.T0)
    trel = IR.relative(f.Tm, f.T0)
    st = IR.solve(cfg, IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), 1))
    assert not st.lost and t.T.tobytes() == IR.output_pose(IR.advance(trel, st.delta), f.Tm).tobytes()
    assert (int(t.result["iterations_run"]), int(t.result["n_corr"]), float(t.result["delta"])) == (1, st.count, st.norm)
    trace = []
    t = IR.track(IC.config(f.K, **IC.LEVELS[1]), f.D, f.M, f.N, f.Tm, f.T0, trace)
    assert [lv for lv, _, _ in trace] == [0, 0] and int(t.result["valid"]) == 1 and int(t.result["level"]) == 0
    assert 16 <= trace[0][1][28] == IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), 16)[28] < IC.config().min_corr
    t, trace = IC.ref("corner")
    assert 3 <= len(trace) <= 19 and int(t.result["level"]) == 2


def test_algorithmic_bytes():
    cfg = IR.config()
    px = 4 * 188 * 120 + 5 * 376 * 240 + 10 * 752 * 480
    assert IR.algorithmic_bytes(cfg, 752, 480, 3) == 3 * (20 * px + 320)
