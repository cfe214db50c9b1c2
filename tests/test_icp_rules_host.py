"""The rule table and the solve table of tests/icp_cases.py on the restatement alone (aria_slam_amd/icp_ref.py). No GPU.

tests/test_gpu_icp_rules.py holds the device to the restatement on these tables; this file shows that the tables ask what
they are there to ask: every test of rule 3 is the first to reject some pixel, every inclusive limit is met at equality and
one ulp beyond, every tie rounds to even, and a copy of the restatement with one test dropped or made strict gives other
integers on the table -- the mistake is made in a copy of the definition, never in the kernel. For rule 5: which pivot
indices lose a frame, `s == thr`, the min_corr boundary, the blind frame and the configuration edges."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC   # noqa: E402
from aria_slam_amd import icp_ref as IR   # noqa: E402


def _values(g, stride=1):
    return [IC.rule_values(g.cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride) for f, trel in zip(g.batch.frames, g.trels)]


def test_census_every_rule_rejects_first_somewhere_and_a_quarter_is_accepted():
    total = np.zeros(IC.ACCEPTED + 1, np.int64)
    for g in IC.rule_cases():
        assert g.batch.W <= 16 and g.batch.H <= 16
        for stride in (1, 2):
            for f, trel, c in zip(g.batch.frames, g.trels, _values(g, stride)):
                ok = IR.jacobians(g.cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)[0]
                assert ((c.code == IC.ACCEPTED).reshape(-1) == ok).all(), f.name       # the census is the restatement's rule 3
                if stride == 1:
                    n = np.bincount(c.code.reshape(-1), minlength=IC.ACCEPTED + 1)
                    print("%-18s %s" % (f.name, " ".join("%3d" % v for v in n)))
                    total += n
    print("first rejections: %s; accepted %d of %d" % (", ".join("%s %d" % kv for kv in zip(IC.RULES, total)), total[-1], total.sum()))
    assert (total[:-1] >= 1).all(), dict(zip(IC.RULES, total))
    assert 4 * total[-1] >= total.sum()
    # a rule that only the table reaches: the rendered scenes never reject by these (the issue's reading of their geometry)
    f = IC.frame("corner")
    seen = np.bincount(IC.rule_census(IC.config(f.K), f.D, f.M, f.N, IR.relative(f.Tm, f.T0), IR.model_rotation(f.Tm)).reshape(-1),
                       minlength=IC.ACCEPTED + 1)
    for name in ("depth_high", "qz", "normal_long", "reach"):
        assert seen[IC.RULES.index(name)] == 0, name


def test_every_hand_written_pixel_decides_as_the_table_says():
    kinds = set()
    for g in IC.rule_cases():
        vals = _values(g)
        for e in g.expect:
            c = vals[e.frame]
            name = "%s (%d, %d)" % (g.batch.frames[e.frame].name, e.v, e.u)
            assert int(c.code[e.v, e.u]) == e.code, (name, (IC.RULES + ("accepted",))[int(c.code[e.v, e.u])])
            for field in ("um", "vm"):
                want = getattr(e, field)
                if want is not None:
                    got = getattr(c, field)[e.v, e.u]
                    assert got == want and np.signbit(got) == np.signbit(np.float32(want)), (name, field, got)
            if e.at is not None:                                      # the compared quantity is exactly the limit, or one ulp past it
                assert getattr(c, e.at[0])[e.v, e.u] == e.at[1], (name, e.at)
            kinds.add((e.kind, e.code == IC.ACCEPTED))
    assert {("eq", True), ("beyond", False), ("tie", True), ("tie", False), ("nonfinite", False), ("first", False)} <= kinds
    # the limits of the issue's list, each met at equality by an accepted pixel and beyond by a rejected one
    even, odd = IC.rule_cases()
    by = {(even.batch.frames[e.frame].name, e.v, e.u): e for e in even.expect}
    cfg = even.cfg
    assert even.batch.frames[0].D[0, 0] == cfg.min_depth and even.batch.frames[0].D[4, 2] == cfg.max_depth
    assert by[("even.dist", 2, 2)].at[1] == cfg.dist_max * cfg.dist_max and by[("even.reach", 2, 2)].at[1] == cfg.reach * cfg.reach
    assert by[("even.model", 4, 4)].at[1] == np.float32(IR.NORMAL_MAX)
    assert np.signbit(by[("even.ties_neg", 0, 0)].um) and by[("even.ties_neg", 0, 0)].code == IC.ACCEPTED
    assert by[("even.ties", 2, 7)].um == even.batch.W and by[("even.ties", 2, 7)].code == IC.RULES.index("right")      # W - 0.5, W even
    assert {(e.um, e.vm) for e in odd.expect if (e.v, e.u) == (4, 6)} == {(odd.batch.W - 1.0, odd.batch.H - 1.0)}    # W - 0.5, W odd
    # ties go both ways in both axes
    ties = [e for g in (even, odd) for e in g.expect if e.kind == "tie" and e.code == IC.ACCEPTED]
    assert any(e.um > e.u for e in ties) and any(e.um < e.u for e in ties) and any(e.vm > e.v for e in ties) and any(e.vm < e.v for e in ties)


def _copy(old=None, new=None):
    """A private copy of icp_ref compiled from its source with `old` (which must occur exactly once) replaced."""
    src = open(IR.__file__).read()
    if old is not None:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    mod = types.ModuleType("aria_slam_amd.icp_ref_copy")
    mod.__file__, mod.__package__ = IR.__file__, "aria_slam_amd"
    exec(compile(src, IR.__file__, "exec"), mod.__dict__)
    return mod


_AWAY = ("        um, vm = np.rint((fx * q[0]) * iz + cx), np.rint((fy * q[1]) * iz + cy)\n",
         "        away = lambda x: np.copysign(np.floor(np.abs(x) + f32(0.5)), x)\n"
         "        um, vm = away((fx * q[0]) * iz + cx), away((fy * q[1]) * iz + cy)\n")
_NLONG = "        ok &= ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) <= f32(NORMAL_MAX)\n"
_DIST = "        ok &= ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= cfg.dist_max * cfg.dist_max\n"
_REACH = "        ok &= ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) <= cfg.reach * cfg.reach\n"
_NZERO = " & ((Nw[:, 0] != 0) | (Nw[:, 1] != 0) | (Nw[:, 2] != 0))"
RULE_MUTANTS = [   # (the rule, what is done to its test, old, new)
    ("depth_low", "dropped", "(d >= cfg.min_depth) & ", ""), ("depth_low", "strict", "d >= cfg.min_depth", "d > cfg.min_depth"),
    ("depth_high", "dropped", " & (d <= cfg.max_depth)", ""), ("depth_high", "strict", "d <= cfg.max_depth", "d < cfg.max_depth"),
    ("qz", "dropped", "        ok &= q[2] > f32(0)\n", ""),
    # without a bounds test the restatement itself would index outside the map: these four are made strict only
    ("left", "strict", "(um >= f32(0))", "(um > f32(0))"), ("right", "strict", "(um <= f32(W - 1))", "(um < f32(W - 1))"),
    ("top", "strict", "(vm >= f32(0))", "(vm > f32(0))"), ("bottom", "strict", "(vm <= f32(H - 1))", "(vm < f32(H - 1))"),
    ("model_depth", "dropped", "(Mz > f32(0)) & ", ""), ("model_depth", "inclusive", "Mz > f32(0)", "Mz >= f32(0)"),
    ("normal_zero", "dropped", _NZERO, ""),
    ("normal_long", "dropped", _NLONG, ""), ("normal_long", "strict", _NLONG, _NLONG.replace("<=", "<")),
    ("dist", "dropped", _DIST, ""), ("dist", "strict", _DIST, _DIST.replace("<=", "<")),
    ("reach", "dropped", _REACH, ""), ("reach", "strict", _REACH, _REACH.replace("<=", "<")),
    ("rintf", "half away from zero", *_AWAY),
    # a NaN fails every comparison: the same tests written as `reject when greater` let it through
    ("normal_long", "passes a NaN", _NLONG, _NLONG.replace("ok &= (", "ok &= ~((").replace("<= f32(NORMAL_MAX)", "> f32(NORMAL_MAX))")),
    ("dist", "passes a NaN", _DIST, _DIST.replace("ok &= (", "ok &= ~((").replace("<= cfg.dist_max * cfg.dist_max", "> cfg.dist_max * cfg.dist_max)")),
]   # (a NaN let through by the depth, q_z, Mz or reach test is rejected by a later one: nothing can see those)


@pytest.mark.parametrize("rule,what,old,new", RULE_MUTANTS, ids=["%s_%s" % (m[0], m[1].replace(" ", "_")) for m in RULE_MUTANTS])
def test_the_rule_table_catches_an_altered_restatement(rule, what, old, new):
    mod = _copy(old, new)
    differ = []
    for g in IC.rule_cases():
        want = IC.rule_systems(g, 1)
        for i, (f, trel) in enumerate(zip(g.batch.frames, g.trels)):
            with np.errstate(all="ignore"):                           # a NaN let through has no integer
                got = mod.system(g.cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), 1)
            if (got != want[i]).any():
                differ.append("%s (%d of 29, count %d for %d)" % (f.name, int((got != want[i]).sum()), int(got[28]), int(want[i][28])))
    print("%s %s: %s" % (rule, what, "; ".join(differ) or "NOT SEEN"))
    assert differ


def test_the_unaltered_copy_gives_the_same_integers_and_every_rule_has_a_mutant():
    mod = _copy()
    for g in IC.rule_cases():
        for stride in (1, 2):
            want = IC.rule_systems(g, stride)
            for i, (f, trel) in enumerate(zip(g.batch.frames, g.trels)):
                assert (mod.system(g.cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride) == want[i]).all()
    assert {m[0] for m in RULE_MUTANTS} == set(IC.RULES) | {"rintf"}
    # the table is not one frame: several frames have correspondences, and stride 2 keeps some of the hand-written pixels
    even = IC.rule_cases()[0]
    assert (IC.rule_systems(even, 1)[:, 28] > 0).sum() >= 8 and (IC.rule_systems(even, 2)[:, 28] > 0).sum() >= 8
    assert (IC.rule_systems(even, 1) != 0).any(axis=0)[:28].all()


# ---- rule 5 ---------------------------------------------------------------------------------------------------------------
def _case(name):
    return {c.name: c for c in IC.solve_cases()}[name]


def test_solve_table_loses_the_first_accumulation_at_every_pivot_index():
    reached = {}
    for c in IC.solve_cases():
        if not c.name.startswith("pivot") or c.name == "pivot0_below":
            continue
        t, trace = IC.solve_ref(c)
        st = trace[0][2]
        assert st.lost and st.count >= c.cfg.min_corr and len(trace) == 1 and int(t.result["valid"]) == 0, c.name
        j = len(st.pivots) - 1
        assert c.name.startswith("pivot%d_" % j), (c.name, st.pivots)
        assert all(p > c.cfg.min_pivot * st.count for p in st.pivots[:-1])
        assert (st.pivots[-1] == 0.0) == c.name.endswith("_zero")        # an exact zero, or a pivot that is something and too small
        assert t.T.tobytes() == np.asarray(c.frame.T0).tobytes() and float(t.result["delta"]) == 0.0 and float(t.result["rms"]) > 0
        reached.setdefault(j, []).append(c.name)
    print("pivot indices at which the first accumulation is lost:", {j: reached[j] for j in sorted(reached)})
    assert sorted(reached) == [0, 1, 2, 3, 4, 5]
    assert sum(1 for j in (1, 2, 3, 4) if any(not n.endswith("_zero") for n in reached[j])) >= 2     # two between 0 and 5 by a threshold


def test_pivot_equal_to_the_threshold_loses_and_one_ulp_less_does_not():
    eq, below = _case("pivot0_equal"), _case("pivot0_below")
    st = IC.solve_ref(eq)[1][0][2]
    assert st.count == 256 and st.pivots == [eq.cfg.min_pivot * 256.0] and st.lost          # s == thr exactly
    assert below.cfg.min_pivot == np.nextafter(eq.cfg.min_pivot, 0.0)
    t, trace = IC.solve_ref(below)
    st = trace[0][2]
    assert len(st.pivots) == 6 and st.pivots[0] > below.cfg.min_pivot * 256.0 and st.pivots[0] == min(st.pivots)
    assert int(t.result["valid"]) == 1 and int(IC.solve_ref(eq)[0].result["valid"]) == 0       # the one ulp is seen in the outputs


def test_min_corr_boundary_blind_frame_and_configuration_edges():
    t, trace = IC.solve_ref(_case("min_corr_equal"))
    assert trace[0][2].count == _case("min_corr_equal").cfg.min_corr == 256 and int(t.result["valid"]) == 1
    t, trace = IC.solve_ref(_case("min_corr_over"))
    assert trace[0][2].lost and trace[0][2].pivots == [] and int(t.result["n_corr"]) == 256 and int(t.result["valid"]) == 0
    c = _case("blind")
    t, trace = IC.solve_ref(c)
    assert set(np.unique(np.nan_to_num(c.frame.D, nan=-1.0))) == {-1.0, 0.0}                  # NaN and 0 only
    assert t.result.tolist() == (0, 1, 0, 0, 0.0, 0.0) and t.T.tobytes() == np.asarray(c.frame.T0).tobytes()
    assert t.T.tobytes() != np.asarray(c.frame.Tm).tobytes()
    c = _case("zero_thresholds")
    t, trace = IC.solve_ref(c)
    assert (c.cfg.min_pivot, c.cfg.eps, c.cfg.iterations) == (0.0, 0.0, (0, 64))
    assert t.result.tolist()[:4] == (1, 64, 256, 1) and [lv for lv, _, _ in trace] == [1] * 64   # eps = 0 never stops a level
    t, trace = IC.solve_ref(_case("skipped_level"))
    assert int(t.result["valid"]) == 1 and 1 < int(t.result["iterations_run"]) < 64 and int(t.result["level"]) == 1


SOLVE_MUTANTS = [("pivot test inclusive", "        if not (s > thr):\n", "        if not (s >= thr):\n", "pivot0_equal"),
                 ("pivot test inclusive at zero", "        if not (s > thr):\n", "        if not (s >= thr):\n", "pivot2_zero"),
                 ("min_corr strict", "    if count < cfg.min_corr:\n", "    if count <= cfg.min_corr:\n", "min_corr_equal"),
                 ("min_corr off by one", "    if count < cfg.min_corr:\n", "    if count < cfg.min_corr - 1:\n", "min_corr_over"),
                 ("eps = 0 stops a level", "            if st.norm < cfg.eps:\n", "            if st.norm < max(cfg.eps, 1e-6):\n", "zero_thresholds")]


@pytest.mark.parametrize("what,old,new,name", SOLVE_MUTANTS, ids=[m[0].replace(" ", "_") for m in SOLVE_MUTANTS])
def test_the_solve_table_catches_an_altered_restatement(what, old, new, name):
    c = _case(name)
    want = IC.solve_ref(c)[0]
    with np.errstate(all="ignore"):
        try:
            got = _copy(old, new).track(c.cfg, c.frame.D, c.frame.M, c.frame.N, c.frame.Tm, c.frame.T0)
            same = got.result.tobytes() == want.result.tobytes() and got.T.tobytes() == want.T.tobytes()
        except (ZeroDivisionError, ValueError):                       # a zero pivot let through divides by zero
            same = False
    assert not same, what


# ---- the large shapes ---------------------------------------------------------------------------------------------------------
def test_batch_of_300_has_valid_lost_masked_and_non_finite_frames_around_index_256():
    cfg, b = IC.batch300()
    poses, recs, invalid = IC.expected(b, cfg)
    gp, gr = IC.guarded_outputs(IC.BIG_N)
    assert len(b.frames) == IC.BIG_N and (b.W, b.H) == (16, 12) and invalid and IC.BIG_NAN > 256
    assert not b.mask[255] and b.mask[256] and not b.mask[257] and not b.mask[5] and not b.mask[299]
    live = [i for i in range(IC.BIG_N) if b.mask[i] and i != IC.BIG_NAN]
    lost = [i for i in live if not recs[i]["valid"]]
    print("batch of 300: %d valid, %d lost (%d of them past 256), iterations %s" %
          (len(live) - len(lost), len(lost), sum(i > 256 for i in lost), np.bincount(recs["iterations_run"][live]).tolist()))
    assert len(lost) >= 20 and any(i < 256 for i in lost) and any(i > 256 for i in lost) and len(live) - len(lost) >= 200
    assert len({poses[i].tobytes() for i in live}) == len(live)                     # 300 different guesses, 300 different answers
    for i in IC.BIG_MASKED:
        assert poses[i].tobytes() == gp[i].tobytes() and recs[i:i + 1].tobytes() == gr[i:i + 1].tobytes()
    assert recs[IC.BIG_NAN:IC.BIG_NAN + 1].tobytes() == bytes(32) and poses[IC.BIG_NAN].tobytes() == gp[IC.BIG_NAN].tobytes()


@pytest.mark.parametrize("w,h", ((IC.STRIP, 1), (1, IC.STRIP)))
def test_strips_have_more_than_half_their_pixels_accepted(w, h):
    cfg, f, trel = IC.strip_case(w, h)
    IR.check_size(w, h)
    with pytest.raises(ValueError):
        IR.check_size(w + (w > 1), h + (h > 1))
    for stride in (1, 16):
        S = IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)
        print("%d x %d stride %d: %d of %d accepted" % (w, h, stride, int(S[28]), IC.STRIP // stride))
        assert 2 * int(S[28]) > IC.STRIP // stride
    trace = []
    t = IR.track(cfg, f.D, f.M, f.N, f.Tm, f.T0, trace)
    assert 2 * trace[0][2].count > IC.STRIP and not trace[0][2].lost and len(trace) >= 2
    assert list(IR.relative(f.Tm, f.T0)) == trel                      # the track starts at the Trel of debug_system
