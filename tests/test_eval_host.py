"""Trajectory evaluation (include/aria_orb_hip.h, "trajectory evaluation"): the parts that need no GPU -- exports and record
layouts, known answers of the NumPy restatement (aria_slam_amd/eval_ref.py) that do not go through its own code path, the
ground-truth loaders, and the kernels' listing."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

EVAL_SYMBOLS = ["aria_eval_default_config", "aria_eval_create", "aria_eval_destroy", "aria_eval_stream", "aria_eval_check",
                "aria_eval_sample_truth_device", "aria_eval_sample_truth", "aria_eval_batch_device", "aria_eval_batch"]
RECORDS = ["aria_eval_config", "aria_eval_truth", "aria_eval_result"]
ULP = 2.0 ** -52


def test_eval_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in EVAL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert aria.HipTrajectoryEvaluator and aria.load_ground_truth_csv
    assert "eval_ref.py" in header and "not pinned" in header[header.index("trajectory evaluation"):]


def test_eval_record_layouts_and_defaults(aria, tmp_path):
    from aria_slam_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aria_orb_hip.h"\nint main(void) { printf("' + "%zu " * len(RECORDS) + '\\n", ' +
                   ", ".join("sizeof(%s)" % r for r in RECORDS) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [24, 136, 200]
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for rec, size in zip(RECORDS, sizes):           # the sizes the header's comments cite
        assert re.search(r"\} %s;\s*/\* %d bytes" % (rec, size), header), rec
    assert C.sizeof(_lib.EvalConfig) == 24
    for struct, dtype, size in ((_lib.EvalTruth, _lib.EVAL_TRUTH_DTYPE, 136), (_lib.EvalResult, _lib.EVAL_RESULT_DTYPE, 200)):
        assert C.sizeof(struct) == dtype.itemsize == size
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
    cfg = _lib.EvalConfig()
    aria.load_library().aria_eval_default_config(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.stream, cfg.align_mode, cfg.rpe_delta) == (24, 0, None, _lib.EVAL_ALIGN_SIM3, 10)
    # the record is the CSV's column order: t, p, q (w, x, y, z), v, b_w, b_a
    assert [n for n, _ in _lib.EvalTruth._fields_] == ["t", "p", "q", "v", "bg", "ba"]


# ---- known answers of the restatement: ATE and RPE ----------------------------------------------------------------------------
def test_ate_and_rpe_by_hand_on_a_12_pose_track():
    """est_i = (1.1 i, 0.5, 0), truth_i = (i, 0, 0): |e_i - g_i|^2 = 0.01 i^2 + 0.25, sum_{i<12} i^2 = 506, so ATE =
    sqrt(0.01 * 506 / 12 + 0.25). With delta = 10 the pairs are i = 10, 11; both deltas are (11, 0, 0) against (10, 0, 0): RPE = 1.
    With delta = 3 there are 9 pairs of difference 0.3: RPE = 0.3. A dozen fp64 operations per term: 16 ulp."""
    from aria_slam_amd import eval_ref as R
    i = np.arange(12.0)
    e = np.stack([1.1 * i, 0.5 + 0 * i, 0 * i], 1)
    g = np.stack([i, 0 * i, 0 * i], 1)
    want = (0.01 * 506 / 12 + 0.25) ** 0.5
    assert abs(R.ate(e, g) - want) <= 16 * ULP * want
    r10, n10 = R.rpe(e, g, 10)
    r3, n3 = R.rpe(e, g, 3)
    assert n10 == 2 and abs(r10 - 1.0) <= 16 * ULP and n3 == 9 and abs(r3 - 0.3) <= 16 * ULP
    res = R.evaluate(e, g, R.ALIGN_NONE, 10)
    assert res["valid"] == 1 and res["n_poses"] == res["n_used"] == 12 and res["n_rpe_pairs"] == 2 and res["align_valid"] == 1
    assert res["ate_raw"] == R.ate(e, g) and res["rpe_raw"] == r10
    # mode none: the aligned figures are the raw ones
    assert abs(res["ate_rmse"] - want) <= 16 * ULP * want and abs(res["rpe_aligned"] - 1.0) <= 16 * ULP
    assert abs(res["ate_max"] - (0.01 * 121 + 0.25) ** 0.5) <= 16 * ULP * 1.3
    # masked poses take no part; an RPE pair needs both of its ends
    mask = np.ones(12, np.uint8)
    mask[[0, 5]] = 0
    want_m = ((0.01 * (506 - 25) + 0.25 * 10) / 10) ** 0.5
    assert abs(R.ate(e, g, mask) - want_m) <= 16 * ULP * want_m
    assert R.rpe(e, g, 10, mask)[1] == 1 and R.rpe(e, g, 5, mask)[1] == 5        # i = 5 and i = 10 lose their ends
    em = e.copy()
    em[[0, 5]] = np.nan                                                          # what a masked pose holds does not matter
    assert R.evaluate(em, g, R.ALIGN_NONE, 10, mask)["ate_raw"] == R.ate(e, g, mask)


def test_empty_conventions_follow_the_reference():
    from aria_slam_amd import eval_ref as R
    e, g, _ = R.make_track("walk", 10, 1)
    assert R.rpe(e, g, 10) == (-1, 0) and R.rpe(e[:3], g[:3], 10) == (-1, 0)       # n <= delta
    assert R.rpe(e, g, 9)[1] == 1
    assert R.ate(e[:0], g[:0]) == -1 and R.ate(e, g, np.zeros(10)) == -1
    res = R.evaluate(e, g, R.ALIGN_SIM3, 10, np.zeros(10))
    assert res["valid"] == 1 and res["ate_raw"] == -1 and res["rpe_raw"] == -1 and res["align_valid"] == 0 and res["n_used"] == 0
    assert res["ate_rmse"] == -1 and res["scale"] == -1
    assert R.evaluate(e, g, R.ALIGN_SIM3, 0)["valid"] == 0                        # delta < 1
    e[4, 1] = np.inf
    assert R.evaluate(e, g)["valid"] == 0


# ---- alignment ---------------------------------------------------------------------------------------------------------------
def _kabsch_numpy(e, g):
    """R, sigma, var by numpy.linalg.svd: another code path to the same definition."""
    x, y = e - e.mean(0), g - g.mean(0)
    Cm = y.T @ x / len(e)
    U, d, Vt = np.linalg.svd(Cm)
    Sg = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    return U @ Sg @ Vt, d, (x * x).sum() / len(e), Sg[2, 2]


@pytest.mark.parametrize("kind", ["walk", "circle", "corridor"])
def test_a_noise_free_similarity_transform_is_recovered(kind):
    """est = R^T (truth - t) / s is rounded once per coordinate, a few ulp of |truth - t| <= 64 m: the estimate is off by about
    4 * 64 * 2^-52 = 6e-14 m. Scale, t and the aligned ATE see that directly (1e-12 with margin for |R mu| and the sums); a
    rotation sees it divided by the spread that determines it, metres for the walk and the circle, the 0.02 .. 0.04 m lateral
    spread of the corridor (1e-12 and 1e-10 in R)."""
    from aria_slam_amd import eval_ref as R
    e, g, (s, Rm, t) = R.make_track(kind, 800, 3, noise=0.0)
    res = R.evaluate(e, g, R.ALIGN_SIM3, 10)
    assert res["align_valid"] == 1
    print(kind, abs(res["scale"] - s), np.abs(res["R"] - Rm).max(), np.abs(res["t"] - t).max(), res["ate_rmse"])
    assert abs(res["scale"] - s) <= 1e-12 and np.abs(res["t"] - t).max() <= 1e-12 * (10 if kind == "corridor" else 1)
    assert np.abs(res["R"] - Rm).max() <= (1e-10 if kind == "corridor" else 1e-12)
    assert 0 <= res["ate_rmse"] <= 1e-12 and res["ate_max"] <= 1e-12 and res["rpe_aligned"] <= 1e-12
    assert abs(np.linalg.det(res["R"]) - 1) <= 1e-14 and np.abs(res["R"] @ res["R"].T - np.eye(3)).max() <= 1e-14
    # rigid mode: scale is 1 exactly, and the rotation is the same one
    rig = R.evaluate(e, g, R.ALIGN_SE3, 10)
    assert rig["scale"] == 1.0 and rig["align_valid"] == 1 and np.array_equal(rig["R"], res["R"])
    # the raw figures are those of computeATE / computeRPE whatever the mode
    assert rig["ate_raw"] == res["ate_raw"] == R.ate(e, g) and rig["rpe_raw"] == res["rpe_raw"]


@pytest.mark.parametrize("kind", ["walk", "circle"])
def test_rotation_agrees_with_numpy_svd_kabsch_on_well_conditioned_tracks(kind):
    """Two backward-stable SVDs of the same well-conditioned 3x3 matrix: the rotations agree to a few ulp times the condition
    of the polar factor, sigma1 / (sigma2 + sigma3) < 20 here -> 1e-13. Singular values to 16 ulp."""
    from aria_slam_amd import eval_ref as R
    e, g, _ = R.make_track(kind, 600, 5, noise=0.02)
    Rn, d, var, _sgn = _kabsch_numpy(e, g)
    res = R.evaluate(e, g)
    assert np.abs(res["R"] - Rn).max() <= 1e-13
    assert np.abs(res["sigma"] - d).max() <= 16 * ULP * d[0]
    assert abs(res["scale"] - d.sum() / var) <= 1e-13


def test_a_mirrored_estimate_gives_a_proper_rotation():
    """est mirrored in z: the best orthogonal map is a reflection, Umeyama's S = diag(1, 1, -1) turns it into the best proper
    rotation and the third singular value enters the scale negatively."""
    from aria_slam_amd import eval_ref as R
    e, g, _ = R.make_track("walk", 400, 7, noise=0.0)
    e = e * [1, 1, -1]
    al = R.umeyama(e, g)
    Rn, d, var, sgn = _kabsch_numpy(e, g)
    assert sgn == -1 and al["det_sign"] == -1 and al["valid"]
    assert abs(np.linalg.det(al["R"]) - 1) <= 1e-14
    assert np.abs(al["R"] - Rn).max() <= 1e-12
    assert abs(al["scale"] - (d[0] + d[1] - d[2]) / var) <= 1e-13 and al["scale"] < (d[0] + d[1] + d[2]) / var
    assert R.evaluate(e, g)["ate_rmse"] > 1e-3                  # a rotation cannot undo a mirror


def test_svd3_factors_the_matrix_itself():
    from aria_slam_amd import eval_ref as R
    rng = np.random.default_rng(2)
    for scale3 in (1.0, 1e-5, 0.0):
        M = rng.normal(size=(3, 3)) @ np.diag([3.0, 1.0, scale3]) @ rng.normal(size=(3, 3))
        A, sg, V = R.svd3(M)
        assert np.abs(M @ V - A).max() <= 1e-14 * np.abs(M).max() and np.abs(V.T @ V - np.eye(3)).max() <= 1e-15 * 8
        d = np.linalg.svd(M, compute_uv=False)
        # relative accuracy of the small singular value too: that is what working on M and not on M^T M buys
        assert sg[0] >= sg[1] >= sg[2] and np.abs(sg[:2] - d[:2]).max() <= 1e-14 * d[0]
        if scale3 == 1e-5:
            assert abs(sg[2] - d[2]) <= 1e-10 * d[2]


@pytest.mark.parametrize("case", ["collinear", "coincident", "n2"])
def test_degenerate_alignment_keeps_the_raw_fields(case):
    from aria_slam_amd import eval_ref as R
    i = np.arange(12.0)
    g = np.stack([i, 0.5 * i, -0.25 * i], 1)
    if case == "collinear":
        e = np.stack([2.0 * i, 0 * i, 0 * i], 1)               # exactly collinear: powers of two, no rounding
    elif case == "coincident":
        e = np.tile([1.0, 2.0, 3.0], (12, 1))
    else:
        e, g = np.array([[0.0, 0, 0], [1, 0, 0]]), np.array([[0.0, 1, 0], [0, 2, 0]])
    for mode in (R.ALIGN_SE3, R.ALIGN_SIM3):
        res = R.evaluate(e, g, mode, 10)
        assert res["valid"] == 1 and res["align_valid"] == 0 and res["n_used"] == len(e)
        assert res["scale"] == -1 and (res["R"] == -1).all() and (res["t"] == -1).all()
        assert res["ate_rmse"] == res["ate_mean"] == res["ate_max"] == res["rpe_aligned"] == -1 and (res["pose_err"] == -1).all()
        assert res["ate_raw"] == R.ate(e, g) > 0 and res["rpe_raw"] == R.rpe(e, g, 10)[0]
    assert R.evaluate(e, g, R.ALIGN_NONE, 10)["align_valid"] == 1


# ---- the sampler -----------------------------------------------------------------------------------------------------------
def _rows():
    rows = np.zeros((4, 17))
    rows[:, 0] = [10.0, 11.0, 13.0, 14.0]
    rows[:, 1:4] = [[0, 0, 0], [1, 2, 3], [3, -2, 7], [4, 4, 4]]
    c, s = np.cos(0.5), np.sin(0.5)
    rows[:, 4:8] = [[1, 0, 0, 0], [0, 1, 0, 0], [-c, -s, 0, 0], [-c, -s, 0, 0]]
    rows[:, 8:17] = np.arange(36.0).reshape(4, 9)
    return rows


def test_sampler_clamps_exact_hits_and_interpolation():
    from aria_slam_amd import eval_ref as R
    rows = _rows()
    q = [5.0, 10.0, 99.0, 14.0, 11.0, 10.5, 12.0]
    out, valid = R.sample_ground_truth(rows, q)
    assert valid.all()
    assert np.array_equal(out[0], rows[0]) and np.array_equal(out[1], rows[0])      # before / at the first row: copied
    assert np.array_equal(out[2], rows[3])                                          # past the end: the last row, its own t
    # an exact hit interpolates with alpha = 1 between its neighbours: (1 - 1) a + 1 b = b, slerp weights 0 and 1
    assert np.array_equal(out[3], rows[3]) and np.array_equal(out[4], rows[1])
    # alpha = 0.5 between rows 0 and 1: the lerp fields by hand; q: (1,0,0,0) and (0,1,0,0) are 90 degrees apart as 4-vectors,
    # th = pi / 2, both weights sin(pi / 4)
    assert out[5, 0] == 10.5 and np.array_equal(out[5, 1:4], [0.5, 1.0, 1.5]) and np.array_equal(out[5, 8:17], (rows[0, 8:] + rows[1, 8:]) / 2)
    assert np.abs(out[5, 4:8] - [0.5 ** 0.5, 0.5 ** 0.5, 0, 0]).max() <= 4 * ULP
    # alpha = 0.5 between rows 1 and 2: d = -sin 0.5 < 0, so the far end is negated: slerp of (0,1,0,0) and (c,s,0,0),
    # which are th = pi / 2 - 0.5 apart; the midpoint is their normalised sum
    assert out[6, 0] == 12.0 and np.array_equal(out[6, 1:4], [2.0, 0.0, 5.0])
    mid = np.array([np.cos(0.5), 1 + np.sin(0.5), 0, 0])
    mid /= np.sqrt(mid @ mid)
    assert np.abs(out[6, 4:8] - mid).max() <= 8 * ULP
    # the near-parallel branch: equal quaternions (d = 1) take the weights 1 - alpha and alpha
    assert np.abs(R.slerp(rows[2, 4:8], rows[3, 4:8], 0.3) - rows[2, 4:8]).max() <= 2 * ULP
    a = np.array([1.0, 0, 0, 0])
    b = np.array([1.0, 1e-9, 0, 0])                  # d = 1 exactly in fp64, not renormalised: plain lerp
    assert np.array_equal(R.slerp(a, b, 0.25), 0.75 * a + 0.25 * b)
    # the same in extended precision
    outl, _ = R.sample_ground_truth(rows, q, np.longdouble)
    assert outl.dtype == np.longdouble and np.abs(outl - out).max() <= 8 * ULP * 36


def test_sampler_refuses_invalid_tables():
    from aria_slam_amd import eval_ref as R
    rows = _rows()
    bad = rows.copy()
    bad[2, 0] = 10.5                                 # decreasing timestamps
    out, valid = R.sample_ground_truth(bad, [10.2, 12.0])
    assert not valid.any() and not out.any()
    bad = rows.copy()
    bad[3, 16] = np.nan
    assert not R.sample_ground_truth(bad, [10.2])[1].any()
    assert not R.sample_ground_truth(rows[:0], [10.2])[1].any()
    out, valid = R.sample_ground_truth(rows, [10.2, np.nan])
    assert list(valid) == [1, 0] and not out[1].any()
    eq = rows.copy()
    eq[1, 0] = 10.0                                  # equal timestamps are not decreasing
    assert R.sample_ground_truth(eq, [10.0, 12.0])[1].all()


# ---- loaders -----------------------------------------------------------------------------------------------------------------
GT_HEADER = "#timestamp, p_RS_R_x [m], p_RS_R_y [m], p_RS_R_z [m], q_RS_w [], q_RS_x [], q_RS_y [], q_RS_z [], v_RS_R_x [m s^-1], " \
            "v_RS_R_y [m s^-1], v_RS_R_z [m s^-1], b_w_RS_S_x [rad s^-1], b_w_RS_S_y [rad s^-1], b_w_RS_S_z [rad s^-1], " \
            "b_a_RS_S_x [m s^-2], b_a_RS_S_y [m s^-2], b_a_RS_S_z [m s^-2]"


def write_gt_csv(path, rows_ns, extra_lines=()):
    """rows_ns: [(timestamp in ns (int), 16 floats)] written in the order given, with comment, short and empty lines between."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    lines = [GT_HEADER]
    for k, (t, vals) in enumerate(rows_ns):
        lines.append("%d," % t + ",".join(repr(float(v)) for v in vals))
        if k < len(extra_lines):
            lines.append(extra_lines[k])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _gt_rows(n=9):
    rng = np.random.default_rng(4)
    t0 = 1403636579763555584
    order = [3, 0, 1, 2, 8, 4, 6, 5, 7][:n]
    return [(t0 + k * 5_000_000, rng.normal(size=16)) for k in order], t0


def test_load_ground_truth_csv(aria, tmp_path):
    rows, t0 = _gt_rows()
    p = str(tmp_path / "gt" / "data.csv")
    write_gt_csv(p, rows, ["# a comment", "", "1403636579763555584,1.0,2.0", "%d,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15" % t0])
    gt = aria.load_ground_truth_csv(p)
    from aria_slam_amd import _lib
    assert gt.dtype == _lib.EVAL_TRUTH_DTYPE and len(gt) == 9               # the 3- and 16-field rows are dropped
    assert np.all(np.diff(gt["t"]) > 0) and gt["t"][0] == t0 * 1e-9
    by_t = {t: v for t, v in rows}
    flat = gt.view(np.float64).reshape(-1, 17)
    for k in range(9):
        assert np.array_equal(flat[k, 1:], by_t[t0 + k * 5_000_000])
    assert np.array_equal(gt["q"][0], by_t[t0][3:7]) and np.array_equal(gt["ba"][0], by_t[t0][13:16])
    # equal timestamps keep their file order (the stable sort)
    write_gt_csv(p, [(t0 + 5_000_000, np.full(16, 1.0)), (t0, np.full(16, 2.0)), (t0 + 5_000_000, np.full(16, 3.0))])
    gt = aria.load_ground_truth_csv(p)
    assert [r["p"][0] for r in gt] == [2.0, 1.0, 3.0]
    open(p, "w").write(GT_HEADER + "\n")
    assert len(aria.load_ground_truth_csv(p)) == 0


@pytest.fixture(scope="module")
def hostlib(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    aria.load_library()
    L = C.CDLL(os.path.join(PKG, "libaria_hip_adapters.so"))
    L.aria_asl_ground_truth.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    return L


def test_asl_sequence_ground_truth(aria, hostlib, tmp_path):
    """AslSequence reads state_groundtruth_estimate0 like load_ground_truth_csv does; the leica0 fallback yields no rows under
    the 17-field rule; a sequence without ground truth still loads."""
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "mav0", "cam0"))
    t0 = 1403636579763555584
    open(os.path.join(root, "mav0", "cam0", "data.csv"), "w").write("#timestamp [ns],filename\n%d,%d.png\n" % (t0, t0))
    buf = np.zeros((64, 17))
    assert hostlib.aria_asl_ground_truth(root.encode(), buf.ctypes.data, 64) == 0          # none: still loads
    os.makedirs(os.path.join(root, "mav0", "leica0"))
    open(os.path.join(root, "mav0", "leica0", "data.csv"), "w").write(
        "#timestamp,p_RS_R_x [m],p_RS_R_y [m],p_RS_R_z [m]\n%d,1.0,2.0,3.0\n%d,1.5,2.0,3.0\n" % (t0, t0 + 5))
    assert hostlib.aria_asl_ground_truth(root.encode(), buf.ctypes.data, 64) == 0          # 4 fields per row: nothing survives
    rows, _ = _gt_rows()
    p = os.path.join(root, "mav0", "state_groundtruth_estimate0", "data.csv")
    write_gt_csv(p, rows, ["# a comment", "", "1403636579763555584,1.0,2.0"])
    n = hostlib.aria_asl_ground_truth(root.encode(), buf.ctypes.data, 64)
    want = aria.load_ground_truth_csv(p)
    assert n == len(want) == 9 and buf[:n].tobytes() == want.tobytes()
    assert hostlib.aria_asl_ground_truth(os.path.join(root, "mav0").encode(), buf.ctypes.data, 64) == 9
    assert hostlib.aria_asl_ground_truth(b"/nonexistent", buf.ctypes.data, 64) == -1


# ---- the kernels' listing and the build ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    path = str(tmp_path_factory.mktemp("eval") / "traj_eval.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "traj_eval.hip")])
    return open(path).read()


@pytest.mark.parametrize("kernel", ["k_truth_scan", "k_truth_sample", "k_traj_eval"])
def test_eval_kernels_cross_compile_without_scratch(listing, kernel):
    body, meta = S.kernel_body(listing, kernel)
    assert len(body) > 30
    assert meta.get("ScratchSize", -1) == 0, meta
    in_loop, outside = S.scratch_accesses(listing, kernel)
    assert not in_loop and not outside
    assert meta.get("LDSByteSize", 0) <= 1024
    hist, _w, _n = S.stats(body)
    float_atomics = [op for op in hist if "atomic" in op and re.search(r"_f(16|32|64)|_pk_", op)]
    assert not float_atomics, float_atomics
    if kernel == "k_traj_eval":
        assert any(op.startswith("v_add_f64") for op in hist)            # fp64 throughout
    print(kernel, len(body), meta)


def test_traj_eval_is_in_the_product_build_reads_no_environment_and_has_no_float_atomics():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "traj_eval.hip" in src_line
    text = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "traj_eval.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    text += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in text)
    assert "getenv" not in text and "atomicAdd" not in text and "atomicMax" not in text and "unsafeAtomic" not in text
    assert set(re.findall(r"\batomic[A-Z]\w*", text)) == {"atomicOr"}      # the integer error word only
    hm = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "src/HipTrajectoryEvaluator.cpp" in hm


def test_eval_selftest_reads_the_ground_truth_like_the_python_loader(aria, hostlib, tmp_path):
    """The CPU part of tests/cpp/eval_selftest.cpp: AslSequence::groundTruth() through the C++ class's own accessors."""
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "mav0", "cam0"))
    t0 = 1403636579763555584
    open(os.path.join(root, "mav0", "cam0", "data.csv"), "w").write("#timestamp [ns],filename\n%d,%d.png\n" % (t0, t0))
    rows, _ = _gt_rows()
    p = os.path.join(root, "mav0", "state_groundtruth_estimate0", "data.csv")
    write_gt_csv(p, rows, ["# a comment", ""])
    exe = os.path.join(ROOT, "build", "eval_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "eval_selftest.cpp"), "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe, "gt", root], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    want = aria.load_ground_truth_csv(p)
    assert lines[0] == "rows 9"
    got = np.array([l.split()[1:] for l in lines[1:]], np.float64)
    assert got.tobytes() == want.tobytes()
