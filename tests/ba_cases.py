"""The case table of the bundle-adjustment stage, shared by the CPU test (tests/test_ba_host.py: it pins the accept/reject
pattern, the margin of every decision and what the table covers, with the restatement alone), the GPU test
(tests/test_gpu_ba.py: the device against ba_ref.optimize at every iteration count up to K) and tools/ba_gap.py (the
tolerance table). A plain module: no fixtures, no pytest.

A case is Case(name, scene, edits, K, note): `scene` are the keyword arguments of ba_ref.random_window (or "exact"),
`edits` names changes made to the generated window (below), PATTERNS[name] is one letter per trial of
ba_ref.optimize(window, K), A accepted and r rejected, in the order they run.

Every run of k iterations is the first k iterations of the run of K > k: the LM state is rebuilt from the window at each
call. So one run of K iterations of the restatement, with its history, is the reference of the device's runs k = 1..K.

The exact case. Identity rotations, camera centres, points and intrinsics that are small dyadic numbers: every projection
is an integer pixel computed without rounding, so chi2 = 0, b = 0, every entry of U and V is exact in any summation order,
every trial is a zero step with rho == 0 exactly, which rho > 0 rejects: ten rejected trials, lambda = lambda0 * 2^55.

GAPS[name][k - 1]: after k iterations, the largest of (a) ba_ref(solver="schur") against ba_ref(solver="full") and (b)
ba_ref(solver="schur") against the same with every sum taken in reversed order, each taken over every pose entry, every
point, lambda and chi2_final -- every difference divided by max(1, |value|), so that one number covers them all. Copied
from the output of tools/ba_gap.py; tests/test_gpu_ba.py allows the device ten times it. GT[name] = the restatement's mean
pose and point errors against the generator's truth (before, after), from the same output."""
import collections
import functools

import numpy as np

from aria_slam_amd import ba_ref as B

Case = collections.namedtuple("Case", "name scene edits K note")

K_ITER = 6
RHO_MIN = 1e-2             # every decision's |rho| is at least this ...
RHO_MARGIN = 1000.0        # ... and this many times the schur-vs-full difference of that trial's rho
EXACT_K = (256.0, 256.0, 320.0, 240.0)

PARTIAL = dict(seed=11, poses=16, points=300, visibility=(2, 16), pixel_noise=0.5, pose_noise=0.05, point_noise=0.2)

CASES = [
    Case("tiny", dict(seed=3, poses=3, points=8), (), 4, "3 poses (2 fixed) x 8 points, all visible"),
    Case("partial", PARTIAL, ("single", "fixed_point", "behind"), K_ITER,
         "2..16 views per point; point 0 keeps one observation, point 1 is fixed at its true place, point 2 starts behind its cameras"),
    Case("stride", dict(seed=5, poses=6, points=1100), (), K_ITER, "more points than two workgroup strides"),
    Case("huber", dict(PARTIAL, outlier_share=0.1), ("single", "fixed_point", "behind"), K_ITER,
         "partial with a tenth of the observations 50..200 px off"),
    Case("motion_only", dict(seed=7, poses=6, points=60, point_noise=0.0), ("fix_points",), 2, "every point fixed"),
    Case("structure_only", dict(seed=8, poses=5, points=70, pose_noise=0.0, n_fixed=5), (), 2,
         "every pose fixed: S is empty"),
    Case("one_fixed", dict(seed=9, poses=5, points=80, n_fixed=1), (), 5, "scale is free; the damping holds it"),
    # rejected trials, found by seed search (tools/ba_gap.py --search)
    Case("reject_first", dict(seed=6, poses=5, points=40, pose_noise=0.1, point_noise=0.3, depth=(0.4, 2.0)), (), K_ITER,
         "the first trial is rejected by its gain"),
    Case("reject_later", dict(seed=15, poses=6, points=30, pose_noise=0.2, point_noise=0.4, depth=(0.5, 3.0), visibility=(2, 6)),
         (), K_ITER, "iteration 2 rejects one trial behind a camera and one by its gain before it accepts"),
    Case("reject_three", dict(seed=23, poses=6, points=30, pose_noise=0.2, point_noise=0.4, depth=(0.5, 3.0), visibility=(2, 6)),
         (), K_ITER, "four rejections in a row: ni reaches 16; a rejection by its gain in iteration 2"),
    Case("reject_behind", dict(seed=26, poses=5, points=40, pose_noise=0.1, point_noise=0.3, depth=(0.4, 2.0)), (), K_ITER,
         "five trials of iterations 5 and 6 put a used observation behind its camera"),
    Case("exact", "exact", (), 5, "rho == 0 in all ten trials; lambda ends at lambda0 * 2^55"),
]
BY_NAME = {c.name: c for c in CASES}
LINEARIZE = ("tiny", "partial", "stride", "huber", "motion_only", "structure_only")
GROUND_TRUTH = ("partial", "huber")
EXEMPT = ("exact",)        # no margin on rho: it is 0 by construction

# ---- the output of tools/ba_gap.py, copied
PATTERNS = {
    "tiny": "AAAA",
    "partial": "AAAAAA",
    "stride": "AAAAAA",
    "huber": "AAAAAA",
    "motion_only": "AA",
    "structure_only": "AA",
    "one_fixed": "AAAAA",
    "reject_first": "rAAAAAA",
    "reject_later": "rArrAAAAA",
    "reject_three": "rrrrArAAAAA",
    "reject_behind": "AAAArrrArrA",
    "exact": "rrrrrrrrrr",
}
GAPS = {    # case: per k = 1.., the largest scaled difference
    "tiny": [7.47e-14, 1.20e-14, 1.66e-14, 1.60e-12],    # AAAA
    "partial": [9.27e-15, 3.42e-15, 3.93e-15, 1.04e-14, 1.84e-14, 2.17e-14],    # AAAAAA
    "stride": [7.29e-15, 1.18e-15, 1.42e-15, 1.43e-15, 1.44e-15, 1.73e-15],    # AAAAAA
    "huber": [2.23e-14, 4.69e-15, 1.30e-14, 8.62e-14, 1.71e-12, 9.02e-13],    # AAAAAA
    "motion_only": [2.86e-15, 3.15e-15],    # AA
    "structure_only": [3.78e-15, 4.84e-15],    # AA
    "one_fixed": [3.40e-15, 5.95e-15, 3.45e-15, 2.80e-15, 7.55e-11],    # AAAAA
    "reject_first": [9.90e-15, 2.93e-14, 4.50e-13, 1.60e-13, 6.10e-14, 7.60e-14],    # rAAAAAA
    "reject_later": [1.50e-12, 1.75e-12, 1.99e-12, 2.54e-12, 5.15e-12, 7.18e-12],    # bAbrAAAAA
    "reject_three": [6.11e-16, 6.94e-16, 1.05e-15, 2.10e-15, 2.61e-14, 4.32e-13],    # bbbbArAAAAA
    "reject_behind": [2.46e-11, 2.21e-11, 2.29e-11, 1.59e-11, 1.25e-11, 1.11e-11],    # AAAAbbbAbbA
}
MIN_RHO = {    # case: smallest |rho| of any decision
    "tiny": 0.457,    # margin 3.49e+09, depth decisions at least 4.82 from min_depth
    "partial": 0.996,    # margin 2.2e+10, depth decisions at least 3.44 from min_depth
    "stride": 0.978,    # margin 1.96e+10, depth decisions at least 3.76 from min_depth
    "huber": 0.916,    # margin 1.38e+12, depth decisions at least 1.87 from min_depth
    "motion_only": 1,    # margin inf, depth decisions at least 3.79 from min_depth
    "structure_only": 0.999,    # margin 2.09e+12, depth decisions at least 3.97 from min_depth
    "one_fixed": 0.429,    # margin 6.77e+08, depth decisions at least 3.91 from min_depth
    "reject_first": 0.958,    # margin 4.94e+11, depth decisions at least 0.000326 from min_depth
    "reject_later": 0.951,    # margin 1.03e+10, depth decisions at least 0.00411 from min_depth
    "reject_three": 0.273,    # margin 6.37e+12, depth decisions at least 0.0575 from min_depth
    "reject_behind": 0.3,    # margin 1.27e+11, depth decisions at least 0.00319 from min_depth
}
GT = {    # case: (mean pose, mean point error) before, after
    "tiny": ((0.0322, 0.07816), (0.008195, 0.1031)),
    "partial": ((0.06757, 0.3488), (0.00743, 0.05804)),
    "stride": ((0.04123, 0.07976), (0.001865, 0.03101)),
    "huber": ((0.06734, 0.3542), (0.007193, 0.2653)),
    "motion_only": ((0.02372, 0), (0.002321, 0)),
    "structure_only": ((0, 0.0776), (0, 0.04474)),
    "one_fixed": ((0.0244, 0.07546), (0.005955, 0.05022)),
    "reject_first": ((0.09847, 0.4198), (0.0005008, 0.004797)),
    "reject_later": ((0.3504, 0.6157), (0.009906, 0.06475)),
    "reject_three": ((0.3422, 0.5917), (0.04386, 0.09366)),
    "reject_behind": ((0.09551, 0.5287), (0.1849, 0.4465)),
}


def exact_window():
    P, N = 4, 12
    poses = np.zeros((P, 3, 4))
    for i in range(P):
        poses[i, :, :3] = np.eye(3)
        poses[i, :, 3] = (-0.5 * i, 0.25 * (i % 2), 0.0)
    X = np.array([[0.25 * (j % 4) - 0.5, 0.5 * (j // 4) - 0.5, (2.0, 4.0, 8.0)[j % 3]] for j in range(N)])
    idx = [(j, i) for j in range(N) for i in range(P)]
    obs = np.zeros(len(idx), B.OBS_DTYPE)
    obs["point"], obs["pose"] = [a for a, _ in idx], [b for _, b in idx]
    r, _Xc = B.residuals(poses.reshape(-1, 12), X, obs, EXACT_K)
    assert np.array_equal(r, np.round(r))              # integer pixels: nothing was rounded
    obs["u"], obs["v"] = r[:, 0], r[:, 1]
    fixed = np.zeros(P, np.uint8)
    fixed[:2] = 1
    return B.make_window(poses.reshape(-1, 12), fixed, X, np.zeros(N, np.uint8), obs, EXACT_K)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(window, truth or None) of a case."""
    c = BY_NAME[name]
    if c.scene == "exact":
        return exact_window(), None
    win, truth = B.random_window(**c.scene)
    obs = win["obs"]
    if "single" in c.edits:                            # point 0 keeps its first observation only
        keep = np.ones(len(obs), bool)
        keep[np.flatnonzero(obs["point"] == 0)[1:]] = False
        obs = obs[keep]
    if "fixed_point" in c.edits:
        win["point_fixed"][1] = 1                      # a landmark: fixed where it is
        win["points"][1] = truth["points"][1]
    if "behind" in c.edits:                            # mirrored through the cameras' plane: every view of it is dropped
        win["points"][2, 2] = -win["points"][2, 2]
    if "fix_points" in c.edits:
        win["point_fixed"][:] = 1
    win["obs"] = obs
    return win, truth


def config(name):
    """(K, huber_px, min_depth) the case runs with."""
    return (EXACT_K if name == "exact" else B.EUROC_K), B.HUBER_DEFAULT, B.MIN_DEPTH_DEFAULT


@functools.lru_cache(maxsize=None)
def reference(name, solver="schur", reverse=False):
    """ba_ref.optimize of a case with its K iterations: (poses, points, result with trace and history)."""
    win, _ = scene(name)
    _K, huber, min_depth = config(name)
    return B.optimize(win, BY_NAME[name].K, solver, huber, min_depth, reverse)


def reference_at(name, k):
    p, x, r = reference(name)
    return B.result_at(r, p, x, k)


def pattern(res):
    return "".join("A" if t["accepted"] else "r" for t in res["trace"])


def scaled(a, b):
    """Largest |a - b| / max(1, |b|) over the entries."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def state_gap(pa, xa, ra, pb, xb, rb, rms=False):
    """The largest scaled difference between two outcomes over poses, points, lambda and chi2_final (and rms_px)."""
    g = max(scaled(pa, pb), scaled(xa, xb), scaled(ra["lambda_"], rb["lambda_"]), scaled(ra["chi2_final"], rb["chi2_final"]))
    return max(g, scaled(ra["rms_px"], rb["rms_px"])) if rms else g


def gap(name, k):
    """GAPS[name][k - 1], measured."""
    def at(ref):
        p, x, r = ref
        return B.result_at(r, p, x, k)
    base = at(reference(name))
    return max(state_gap(*at(reference(name, "full")), *base), state_gap(*at(reference(name, "schur", True)), *base))


def decision_margins(name):
    """(the smallest |rho| / |rho - rho of the full solver| over the trials decided by their gain, the smallest distance
    from min_depth of the depth that decides a trial). inf where nothing differs."""
    tr, tf = reference(name)[2]["trace"], reference(name, "full")[2]["trace"]
    margin, zdist = np.inf, np.inf
    for a, b in zip(tr, tf):
        if not a["solved"]:
            continue
        zdist = min(zdist, abs(a["min_z"] - config(name)[2]))
        if np.isfinite(a["rho"]) and np.isfinite(b["rho"]) and a["rho"] != b["rho"]:
            margin = min(margin, abs(a["rho"]) / abs(a["rho"] - b["rho"]))
    return margin, zdist


# ---- invalid windows: one for each validation rule ---------------------------------------------------------------------------
def invalid_windows():
    """[(name, window)]: `tiny` with one rule broken each. Counts the records do not have travel as n_poses / n_obs keys."""
    base, _ = scene("tiny")
    out = []

    def edit(name, fn):
        w = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        fn(w)
        out.append((name, w))

    edit("point_index", lambda w: w["obs"]["point"].__setitem__(5, len(w["points"])))
    edit("pose_index", lambda w: w["obs"]["pose"].__setitem__(5, -1))
    edit("order", lambda w: w["obs"].__setitem__([3, 4], w["obs"][[4, 3]]))
    edit("duplicate", lambda w: w["obs"].__setitem__(4, w["obs"][3]))
    edit("too_many_poses", lambda w: w.update(poses=np.tile(w["poses"][:1], (17, 1)), pose_fixed=np.ones(17, np.uint8)))
    edit("negative_count", lambda w: w.update(n_obs=-1))
    edit("pose_nan", lambda w: w["poses"].__setitem__((2, 7), np.nan))
    edit("point_inf", lambda w: w["points"].__setitem__((3, 1), np.inf))
    edit("pixel_nan", lambda w: w["obs"]["u"].__setitem__(6, np.nan))
    return out


# ---- a chain for the track builder ---------------------------------------------------------------------------------------------
def generated_chain(seed=21, n=260, frames=5):
    """A 3-D scene seen by five frames: four pairs. Point i is keypoint perm[f][i] of frame f; pair q matches frame q (view 1,
    the query side) to frame q + 1. A share of every pair's matches is left out (broken tracks), and pair 2 holds one view-1
    keypoint twice (the lower match index wins)."""
    from aria_slam_amd import _lib
    rng = np.random.default_rng(seed)
    win, truth = B.random_window(seed, poses=frames, points=n, pixel_noise=0.3)
    tp, X = truth["poses"].reshape(-1, 3, 4), truth["points"]
    o = win["obs"]
    px = np.stack([o["u"], o["v"]], axis=1).reshape(n, frames, 2)
    perm = [rng.permutation(n) for _ in range(frames)]
    kps = np.zeros((frames, n), _lib.KP_DTYPE)
    for f in range(frames):
        kps[f]["x"][perm[f]], kps[f]["y"][perm[f]] = px[:, f, 0], px[:, f, 1]
        kps[f]["size"], kps[f]["response"] = 31.0, 1.0
    cap = n
    matches, nm = np.zeros((frames - 1, cap), _lib.MATCH_DTYPE), np.zeros(frames - 1, np.int32)
    for q in range(frames - 1):
        keep = rng.permutation(n)[:int(0.8 * n)]
        matches[q]["query_idx"][:len(keep)], matches[q]["train_idx"][:len(keep)] = perm[q][keep], perm[q + 1][keep]
        nm[q] = len(keep)
    matches[2][7] = (matches[2][3]["query_idx"], matches[2][8]["train_idx"], 0)       # the same view-1 keypoint again, later
    ext = np.stack([np.concatenate([tp[q].reshape(-1), tp[q + 1].reshape(-1)]) for q in range(frames - 1)])
    return kps, matches, nm, ext, win, truth
