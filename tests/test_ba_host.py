"""Local bundle adjustment (include/aria_orb_hip.h, "local bundle adjustment"): the parts that need no GPU -- exports and
layouts, the NumPy restatement (aria_slam_amd/ba_ref.py: the Jacobians against central differences, the Schur step against
the undivided solve, validation, the track builder on a hand-built chain), the case table (tests/ba_cases.py: pattern,
margin and coverage, proved with the restatement alone) and the kernel's listing."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_cases as BC          # noqa: E402
import isa_kernel_stats as S   # noqa: E402

BA_SYMBOLS = ["aria_ba_window_from_chain_device", "aria_ba_default_config", "aria_ba_create", "aria_ba_destroy", "aria_ba_stream", "aria_ba_check",
              "aria_ba_optimize", "aria_ba_optimize_batch_device", "aria_ba_debug_linearize"]


def test_ba_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in BA_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipBundleAdjuster


def test_ba_record_layouts_and_defaults(aria, tmp_path):
    from aria_slam_amd import _lib, ba_ref as B
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aria_orb_hip.h"\nint main(void) { printf("%zu %zu %zu %d\\n", '
                   'sizeof(aria_ba_config), sizeof(aria_ba_obs), sizeof(aria_ba_result), ARIA_BA_MAX_POSES); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    cfg_size, obs_size, res_size, max_poses = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                              check=True).stdout.split()]
    assert C.sizeof(_lib.BaConfig) == cfg_size == 72
    assert _lib.BA_OBS_DTYPE.itemsize == obs_size == 16 and B.OBS_DTYPE == _lib.BA_OBS_DTYPE
    assert _lib.BA_RESULT_DTYPE.itemsize == res_size == 56
    assert max_poses == B.MAX_POSES == 16
    cfg = _lib.BaConfig()
    aria.load_library().aria_ba_default_config(C.byref(cfg))
    assert cfg.struct_size == 72 and cfg.max_iterations == 10 and cfg.max_windows == 256
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == B.EUROC_K
    assert cfg.huber_px == B.HUBER_DEFAULT == np.sqrt(5.991) and cfg.min_depth == B.MIN_DEPTH_DEFAULT == 1e-6


# ---- ba_ref: the pieces -----------------------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences():
    from aria_slam_amd import ba_ref as B
    win, _ = B.random_window(2, poses=4, points=10, depth=(1.0, 6.0))
    Jc, Jp = B.jacobians(win["poses"], win["points"], win["obs"], win["K"])
    h, worst = 1e-6, 0.0
    for o in range(len(win["obs"])):
        ob = win["obs"][o:o + 1]
        num_c, num_p = np.zeros((2, 6)), np.zeros((2, 3))
        for k in range(6):
            d = np.zeros((len(win["poses"]), 6))
            d[ob["pose"][0], k] = h
            rp = B.residuals(B.apply_update(win["poses"], win["points"], d, 0.0)[0], win["points"], ob, win["K"])[0]
            rm = B.residuals(B.apply_update(win["poses"], win["points"], -d, 0.0)[0], win["points"], ob, win["K"])[0]
            num_c[:, k] = (rp - rm)[0] / (2 * h)
        for k in range(3):
            d = np.zeros_like(win["points"])
            d[ob["point"][0], k] = h
            rp = B.residuals(win["poses"], win["points"] + d, ob, win["K"])[0]
            rm = B.residuals(win["poses"], win["points"] - d, ob, win["K"])[0]
            num_p[:, k] = (rp - rm)[0] / (2 * h)
        worst = max(worst, np.abs(num_c - Jc[o]).max() / np.abs(Jc[o]).max(), np.abs(num_p - Jp[o]).max() / np.abs(Jp[o]).max())
    # central differences at h = 1e-6 carry h^2 truncation and eps / h rounding: about 1e-10 of the largest entry
    assert worst < 1e-7, worst


def test_huber_terms_and_the_used_mask():
    from aria_slam_amd import ba_ref as B
    r = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 4.0]])
    w, c, e2 = B.huber_terms(r, 2.0)
    assert np.array_equal(w, [1.0, 1.0, 0.4]) and np.array_equal(c, [0.0, 1.0, 16.0]) and np.array_equal(e2, [0.0, 1.0, 25.0])
    w, c, _ = B.huber_terms(r, 0.0)                    # off
    assert np.array_equal(w, [1, 1, 1]) and np.array_equal(c, [0.0, 1.0, 25.0])
    win, _ = BC.scene("partial")
    used = B.used_mask(win)
    dropped = win["obs"]["point"][~used]
    assert len(dropped) >= 2 and set(dropped) == {2}            # the point behind its cameras, every view of it
    _fp, fpts = B.free_sets(win, used)
    assert not {0, 1, 2} & set(fpts.tolist()) and len(fpts) == len(win["points"]) - 3


def test_validation_rules():
    from aria_slam_amd import ba_ref as B
    good, _ = BC.scene("tiny")
    assert B.check_window(good)
    bad = BC.invalid_windows()
    assert [n for n, _ in bad] == ["point_index", "pose_index", "order", "duplicate", "too_many_poses", "negative_count",
                                   "pose_nan", "point_inf", "pixel_nan"]
    for name, w in bad:
        if "n_obs" in w:
            continue                                            # a count: the arrays of the restatement cannot carry it
        assert not B.check_window(w), name
        p, x, r = B.optimize(w, 3)
        assert (r["valid"], r["stop_reason"], r["trials"]) == (0, B.STOP_INVALID, 0), name
        assert p.tobytes() == w["poses"].tobytes() and x.tobytes() == w["points"].tobytes()


# ---- the case table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in BC.CASES])
def test_case_decisions_cannot_hang_on_a_summation_order(name):
    """The same pattern under both solvers and both orders; every decision by gain has |rho| >= 1e-2 and at least 1000
    times the solvers' difference; every decision by depth is far from min_depth."""
    runs = [BC.reference(name), BC.reference(name, "full"), BC.reference(name, "schur", True)]
    pats = [BC.pattern(r[2]) for r in runs]
    assert pats[0] == pats[1] == pats[2] == BC.PATTERNS[name], pats
    assert [t["solved"] for t in runs[0][2]["trace"]] == [t["solved"] for t in runs[1][2]["trace"]]
    if name in BC.EXEMPT:
        assert all(t["rho"] == 0.0 and t["solved"] for r in runs for t in r[2]["trace"])
        return
    rhos = [abs(t["rho"]) for t in runs[0][2]["trace"] if np.isfinite(t["rho"])]
    assert min(rhos) >= BC.RHO_MIN and min(rhos) == pytest.approx(BC.MIN_RHO[name], rel=5e-3)
    margin, zdist = BC.decision_margins(name)
    assert margin >= BC.RHO_MARGIN, margin
    assert zdist >= 1e-4, zdist                      # depths are of order 1 here: 1e-4 is twelve decades above their rounding


@pytest.mark.parametrize("name", [c.name for c in BC.CASES if c.name not in BC.EXEMPT])
def test_schur_equals_full_to_the_gap_table(name):
    """GAPS is a measurement of rounding, and another BLAS rounds elsewhere: the re-measured gap is held to the allowance the
    device gets, ten times the table."""
    c = BC.BY_NAME[name]
    assert len(BC.GAPS[name]) == c.K
    for k in range(1, c.K + 1):
        assert 0 < BC.GAPS[name][k - 1] < 1e-9
        assert BC.gap(name, k) <= 10 * BC.GAPS[name][k - 1], (k, BC.gap(name, k))
    _p, _x, r = BC.reference(name)
    assert r["chi2_final"] < r["chi2_initial"] and r["iterations_done"] == c.K and r["stop_reason"] == 0
    chi2 = [r["chi2_initial"]] + [h["chi2"] for h in r["history"]]
    assert all(b < a for a, b in zip(chi2, chi2[1:]))


def test_the_table_covers_what_it_claims():
    from aria_slam_amd import ba_ref as B
    sc = {c.name: BC.scene(c.name)[0] for c in BC.CASES}
    assert (len(sc["tiny"]["poses"]), len(sc["tiny"]["points"]), int(sc["tiny"]["pose_fixed"].sum())) == (3, 8, 2)
    assert len(sc["tiny"]["obs"]) == 24
    p = sc["partial"]
    per = np.bincount(p["obs"]["point"], minlength=300)
    assert len(p["poses"]) == 16 and len(p["points"]) == 300 and per[0] == 1 and per[3:].min() >= 2 and per.max() == 16
    assert p["point_fixed"][1] == 1 and p["point_fixed"].sum() == 1
    assert (len(sc["stride"]["poses"]), len(sc["stride"]["points"])) == (6, 1100) and 1100 > 2 * 512
    r, _ = B.residuals(BC.scene("huber")[1]["poses"], BC.scene("huber")[1]["points"], sc["huber"]["obs"], sc["huber"]["K"])
    gross = np.sqrt((r * r).sum(1)) > 40
    assert 0.08 < gross.mean() < 0.12
    assert sc["motion_only"]["point_fixed"].all() and not sc["structure_only"]["pose_fixed"].min() == 0
    assert sc["one_fixed"]["pose_fixed"].sum() == 1
    # the rejected-trial path: at the first trial, later, ni reaching 8, behind a camera
    pats = BC.PATTERNS
    assert pats["reject_first"].startswith("rA") and "Ar" in pats["reject_later"] and "rrr" in pats["reject_three"]
    behind = [t for t in BC.reference("reject_behind")[2]["trace"] if t["solved"] and not t["accepted"] and t["min_z"] <= 1e-6]
    assert len(behind) >= 1 and all(t["chi2_new"] == np.inf for t in behind)
    by_gain = [t for t in BC.reference("reject_first")[2]["trace"][:1] if t["min_z"] > 1e-6 and t["rho"] < 0]
    assert len(by_gain) == 1
    assert sum(len(set(x)) == 2 for x in pats.values()) >= 3
    # exact: ten zero steps
    pe, xe, re_ = BC.reference("exact")
    assert BC.pattern(re_) == "r" * 10 and re_["chi2_initial"] == 0.0 and re_["stop_reason"] == B.STOP_TRIALS
    assert re_["lambda_"] == re_["trace"][0]["lambda_"] * 2.0 ** 55 and re_["trace"][0]["lambda_"] > 0


@pytest.mark.parametrize("name", BC.GROUND_TRUTH)
def test_ground_truth_figures_are_the_restatements(name):
    from aria_slam_amd import ba_ref as B
    win, truth = BC.scene(name)
    p, x, _r = BC.reference(name)
    before, after = B.truth_errors(win["poses"], win["points"], truth, win), B.truth_errors(p, x, truth, win)
    assert before == pytest.approx(BC.GT[name][0], rel=2e-3) and after == pytest.approx(BC.GT[name][1], rel=2e-3)
    assert after[0] < 0.2 * before[0] and after[1] < before[1]


# ---- the track builder --------------------------------------------------------------------------------------------------------------
def _chain():
    """Three pairs over four frames. Keypoint k of frame f sits at pixel (100 f + k, 50 f + 2 k)."""
    from aria_slam_amd._lib import KP_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE
    stride, cap = 6, 5
    frames = np.zeros((4, stride), KP_DTYPE)
    for f in range(4):
        frames[f]["x"], frames[f]["y"] = 100 * f + np.arange(stride), 50 * f + 2 * np.arange(stride)
    kp1, kp2 = frames[:3].copy(), frames[1:].copy()
    n1 = n2 = np.array([6, 6, 6], np.int32)
    matches = np.zeros((3, cap), MATCH_DTYPE)
    nm = np.array([3, 4, 2], np.int32)
    matches[0, :3] = [(0, 1, 0), (2, 3, 0), (4, 5, 0)]
    matches[1, :4] = [(1, 2, 0), (3, 0, 0), (3, 4, 0), (5, 5, 0)]      # view-1 index 3 twice: the lower match index wins
    matches[2, :2] = [(2, 4, 0), (5, 1, 0)]
    arena = np.zeros(6, MAP_POINT_DTYPE)
    #            pair idx1 idx2
    rows = [(9, 0, 0), (10, 0, 1), (10, 2, 3), (11, 3, 0), (10, 4, 5), (12, 2, 4)]
    for k, (pair, i1, i2) in enumerate(rows):
        arena[k]["pair"], arena[k]["idx1"], arena[k]["idx2"], arena[k]["X"] = pair, i1, i2, (k, 2 * k, 3 * k + 1)
    return arena, kp1, n1, kp2, n2, matches, nm


def test_window_from_chain_on_a_hand_built_chain():
    from aria_slam_amd import ba_ref as B
    arena, kp1, n1, kp2, n2, matches, nm = _chain()
    w = B.window_from_chain(arena, 10, 3, kp1, n1, kp2, n2, matches, nm, 8, 32)
    assert w["error"] == 0 and w["n_points"] == 5 and list(w["point_src"]) == [1, 2, 3, 4, 5]
    assert np.array_equal(w["points"], arena["X"][1:])
    px = lambda f, k: (100.0 * f + k, 50.0 * f + 2.0 * k)    # noqa: E731
    want = [
        # arena 1, pair 10: 0 -> 1, pair 11 match (1, 2), pair 12 match (2, 4): a full track
        (0, 0) + px(0, 0), (0, 1) + px(1, 1), (0, 2) + px(2, 2), (0, 3) + px(3, 4),
        # arena 2, pair 10: 2 -> 3, pair 11 has 3 twice: match 1 (3 -> 0) wins, pair 12 has no match from 0: broken
        (1, 0) + px(0, 2), (1, 1) + px(1, 3), (1, 2) + px(2, 0),
        # arena 3, pair 11: 3 -> 0, no match from 0 in pair 12
        (2, 1) + px(1, 3), (2, 2) + px(2, 0),
        # arena 4, pair 10: 4 -> 5, pair 11 match (5, 5), pair 12 match (5, 1)
        (3, 0) + px(0, 4), (3, 1) + px(1, 5), (3, 2) + px(2, 5), (3, 3) + px(3, 1),
        # arena 5, pair 12: 2 -> 4
        (4, 2) + px(2, 2), (4, 3) + px(3, 4),
    ]
    assert w["n_obs"] == len(want) and w["obs"].tobytes() == np.array(want, B.OBS_DTYPE).tobytes()
    key = w["obs"]["point"].astype(np.int64) * 16 + w["obs"]["pose"]
    assert np.all(key[1:] > key[:-1])                           # sorted by construction
    # the capacities and an index out of range: a deferred error, counts 0
    assert B.window_from_chain(arena, 10, 3, kp1, n1, kp2, n2, matches, nm, 4, 32)["error"] == 2
    over = B.window_from_chain(arena, 10, 3, kp1, n1, kp2, n2, matches, nm, 8, 14)
    assert over["error"] == 2 and over["n_points"] == 0 and over["n_obs"] == 0
    bad = matches.copy()
    bad[1, 3]["train_idx"] = 6
    assert B.window_from_chain(arena, 10, 3, kp1, n1, kp2, n2, bad, nm, 8, 32)["error"] == 1
    arena2 = arena.copy()
    arena2[2]["idx2"] = 6
    assert B.window_from_chain(arena2, 10, 3, kp1, n1, kp2, n2, matches, nm, 8, 32)["error"] == 1
    # a window of two pairs sees the same tracks cut at its last frame
    w2 = B.window_from_chain(arena, 10, 2, kp1[:2], n1[:2], kp2[:2], n2[:2], matches[:2], nm[:2], 8, 32)
    assert w2["n_points"] == 4 and w2["n_obs"] == 11 and w2["obs"]["pose"].max() == 2


# ---- the kernel's listing and the build -----------------------------------------------------------------------------------------------
def _listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "ba_schur.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "ba_schur.hip")])
    return open(path).read()


def test_ba_kernel_cross_compiles_without_scratch():
    """Every LM iteration and trial of a window lives in k_ba_lm: the whole kernel has no scratch, and S fits the LDS."""
    text = _listing()
    body, meta = S.kernel_body(text, "k_ba_lm")
    assert len(body) > 500
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(text, "k_ba_lm")
    assert not in_loop and not outside
    assert 96 * 96 * 8 <= meta.get("LDSByteSize", 0) <= 160 * 1024
    assert meta.get("Occupancy", 0) >= 2                        # 512 lanes: two waves per SIMD


def test_ba_schur_is_in_the_product_build_and_has_no_float_atomics():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "ba_schur.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "ba_schur.hip")).read()
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "solver_device.h"))
    assert "getenv" not in src
    # the only atomics are integer ones: the count of the used observations, the track builder's lowest match index
    # (a minimum) and the error word
    atomics = re.findall(r"atomic\w+\(&?\s*([\w.\[\]>-]+)", src)
    assert atomics and all(a.startswith(("L.nused", "A.err", "tab[")) for a in atomics), atomics
    assert "cooperative" not in src and "grid.sync" not in src and "hipLaunchCooperativeKernel" not in src
    flags = [ln for ln in mk.splitlines() if ln.startswith("FLAGS :=")][0]
    assert "-ffp-contract=off" in flags
