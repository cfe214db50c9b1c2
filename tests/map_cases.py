"""Inputs shared by the point-map tests (tests/test_map_host.py, tests/test_gpu_map.py, tests/test_gpu_map_scale.py) and
tools/map_gap.py: the rigs, every scene on which the device's float fields are compared with the restatement, the
restatement's two runs of a scene (fp64 and np.longdouble), the distance of a run's tested quantities to their thresholds,
the many-pair batch of the scan tests and the non-finite keypoint cases. CPU only."""
import numpy as np

EXT = np.longdouble
SCENES = ["ref0", "ref1", "ref2", "ref3", "edges", "scale0", "scale1", "scale2", "scale3"]

# the many-pair batch: more than two rounds of k_map_scan's 1024
SCALE_PAIRS, SCALE_CAP, SCALE_BASE = 2600, 24, 100
SCALE_COUNTS = (0, 5, 7, 8, 12, 16, 24)                  # 5 and 7: below the 8-match gate
SCALE_FULL = (200, 1500, 1700, 2300)                     # pairs given 24 matches: the tests plant at / cut before them


def views(k):
    """World-to-camera extrinsics of two views: four rigs with rotation and a baseline of 1.5-2.5."""
    from aria_slam_amd import map_ref as M
    R1 = M.rot([0.1 * k, 1, 0.2], 3 * k)
    E1 = M.extrinsics(R1, [0.3 * k, -0.1, 0.2])
    R2 = M.rot([0.2, 1, 0.1 * k], -4 - k) @ R1
    E2 = M.extrinsics(R2, [0.3 * k - 1.5 - 0.3 * k * k, 0.2, 0.3])
    return E1, E2


def ref_scene(k):
    """Scene k of test_against_map_ref: (kq, kt, matches, E1, E2)."""
    from aria_slam_amd import map_ref as M
    E1, E2 = views(k)
    kq, kt, m, _, _ = M.synth_scene(50 + k, 2000, E1, E2, outlier_frac=0.2, noise_px=1.0, depth=(0.5, 60.0))
    return kq, kt, m, E1, E2


def edges_pairs():
    """The four pairs of test_edges (pair 0 without matches), all on rig 1."""
    from aria_slam_amd import map_ref as M
    E1, E2 = views(1)
    pairs = []
    for k in range(4):
        kq, kt, m, _, _ = M.synth_scene(70 + k, 200, E1, E2, depth=(1.0, 8.0))
        pairs.append((kq, kt, m, E1, E2))
    pairs[0] = (pairs[0][0][:0], pairs[0][1][:0], pairs[0][2][:0], E1, E2)
    return pairs


def relative_pose(E1, E2):
    """View 2 relative to view 1: (R, t) with x2 = R x1 + t."""
    R = E2[:, :3] @ E1[:, :3].T
    return R, E2[:, 3] - R @ E1[:, 3]


_scale = None


def scale_batch():
    """The batch of the scan tests: SCALE_PAIRS pairs over the four rigs (pair p on rig p % 4), SCALE_CAP slots each, match
    counts drawn from SCALE_COUNTS, 20 % random-pixel outliers. The train keypoints of a pair are stored in reverse, so
    idx1 != idx2. Returns a dict of host arrays: kq, kt (P, cap) KP_DTYPE, mm (P, cap) MATCH_DTYPE, n (P,) int32, ext (P, 24)."""
    global _scale
    if _scale is not None:
        return _scale
    from aria_slam_amd import map_ref as M
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE
    P, cap = SCALE_PAIRS, SCALE_CAP
    n = np.random.default_rng(7).choice(SCALE_COUNTS, P).astype(np.int32)
    n[list(SCALE_FULL)] = cap
    kq, kt = np.zeros((P, cap), KP_DTYPE), np.zeros((P, cap), KP_DTYPE)
    mm = np.zeros((P, cap), MATCH_DTYPE)
    ext = np.zeros((P, 24))
    for k in range(4):
        E1, E2 = views(k)
        rows = np.arange(k, P, 4)
        a, b, _, _, _ = M.synth_scene(300 + k, len(rows) * cap, E1, E2, outlier_frac=0.2, depth=(1.0, 30.0))
        kq[rows], kt[rows] = a.reshape(-1, cap), b.reshape(-1, cap)
        ext[rows, :12], ext[rows, 12:] = E1.reshape(-1), E2.reshape(-1)
    for p in range(P):
        kt[p, :n[p]] = kt[p, :n[p]][::-1].copy()
        mm[p, :n[p]]["query_idx"] = np.arange(n[p])
        mm[p, :n[p]]["train_idx"] = n[p] - 1 - np.arange(n[p])
        mm[p, :n[p]]["distance"] = 1.0
        kq[p, n[p]:], kt[p, n[p]:] = 0, 0
    _scale = dict(kq=kq, kt=kt, mm=mm, n=n, ext=ext)
    return _scale


def scale_rig(k):
    """The matches of rig k of scale_batch in pair order, pairs below the 8-match gate left out:
    (pair (N,), match (N,), idx1 (N,), idx2 (N,), x1 (N, 2), x2 (N, 2), E1, E2); pair is the batch position."""
    b = scale_batch()
    pair, match = [], []
    for p in range(k, SCALE_PAIRS, 4):
        if b["n"][p] >= 8:
            pair.append(np.full(b["n"][p], p))
            match.append(np.arange(b["n"][p]))
    pair, match = np.concatenate(pair), np.concatenate(match)
    i1, i2 = b["mm"]["query_idx"][pair, match], b["mm"]["train_idx"][pair, match]
    x1 = np.stack([b["kq"]["x"][pair, i1], b["kq"]["y"][pair, i1]], 1)
    x2 = np.stack([b["kt"]["x"][pair, i2], b["kt"]["y"][pair, i2]], 1)
    E1, E2 = views(k)
    return pair, match, i1, i2, x1, x2, E1, E2


def pixels(kq, kt, m):
    """(x1, x2) of a match list whose query side is view 1."""
    return (np.stack([kq["x"][m["query_idx"]], kq["y"][m["query_idx"]]], 1),
            np.stack([kt["x"][m["train_idx"]], kt["y"][m["train_idx"]]], 1))


def scene_inputs(name):
    """(x1, x2, E1, E2) of a scene of SCENES, as triangulate_points takes them."""
    from aria_slam_amd import map_ref as M
    if name.startswith("ref"):
        kq, kt, m, E1, E2 = ref_scene(int(name[3:]))
        return pixels(kq, kt, m) + (E1, E2)
    if name == "edges":                                   # pair 3 under its pose record: the world frame is view 1's
        kq, kt, m, E1, E2 = edges_pairs()[3]
        return pixels(kq, kt, m) + (M.extrinsics(np.eye(3), [0, 0, 0]), M.extrinsics(*relative_pose(E1, E2)))
    return scale_rig(int(name[5:]))[4:]


def run(x1, x2, E1, E2, dtype, K=None, **th):
    """One run of the restatement in `dtype`: dict(keep (N,) bool, X (N, 3), err (N, 2), quality (N,), margin (N,)), the float
    fields in dtype. margin: the smallest relative distance of a point's tested quantities -- |w| of the homogeneous
    point against 1e-10, the two depths against min and max, the parallax, the two reprojection errors -- to their
    thresholds, in this run's arithmetic (NaN quantities do not count)."""
    from aria_slam_amd import map_ref as M
    K = M.EUROC_K if K is None else K
    th = dict(M.DEFAULTS, **th)
    reason, X, err = M.triangulate_points(x1, x2, E1, E2, K, dtype=dtype, **th)
    E1, E2 = M.as_extrinsics(E1, dtype), M.as_extrinsics(E2, dtype)
    with np.errstate(all="ignore"):
        z1 = X[:, 0] * E1[2, 0] + X[:, 1] * E1[2, 1] + X[:, 2] * E1[2, 2] + E1[2, 3]
        z2 = X[:, 0] * E2[2, 0] + X[:, 1] * E2[2, 1] + X[:, 2] * E2[2, 2] + E2[2, 3]
        r1, r2 = X + E1[:, :3].T @ E1[:, 3], X + E2[:, :3].T @ E2[:, 3]
        cosp = (r1 * r2).sum(1) / np.sqrt((r1 * r1).sum(1) * (r2 * r2).sum(1))
        par = np.arccos(np.minimum(1.0, np.abs(cosp))) * 180.0 / np.arccos(dtype(-1))
        w = 1.0 / np.sqrt(1.0 + (X * X).sum(1))           # |X[3]| of the unit homogeneous point
        q = [(w, M.W_EPS), (z1, th["min_depth"]), (z1, th["max_depth"]), (z2, th["min_depth"]), (z2, th["max_depth"]),
             (par, th["min_parallax"]), (err[:, 0], th["max_reproj"]), (err[:, 1], th["max_reproj"])]
        margin = np.stack([np.abs(v - t) / t for v, t in q])
        margin = np.where(np.isnan(margin), np.inf, margin).min(axis=0)
        quality = 1.0 / (err[:, 0] + err[:, 1] + 0.1)
    return dict(keep=reason == M.KEPT, X=X, err=err, quality=quality, margin=margin)


_runs = {}


def ref_runs(name):
    """(fp64 run, extended run) of a scene, computed once."""
    if name not in _runs:
        args = scene_inputs(name)
        _runs[name] = (run(*args, np.float64), run(*args, EXT))
    return _runs[name]


def gap(name):
    """GAP of a scene: (X relative, err absolute, quality relative), the largest difference between the fp64 and the extended
    run over the points both keep; and the smallest margin of the extended run."""
    a, b = ref_runs(name)
    s = a["keep"] & b["keep"]
    gx = (np.sqrt(((a["X"][s] - b["X"][s]) ** 2).sum(1)) / np.sqrt((b["X"][s] ** 2).sum(1))).max()
    ge = np.abs(a["err"][s] - b["err"][s]).max()
    gq = (np.abs(a["quality"][s] - b["quality"][s]) / b["quality"][s]).max()
    return float(gx), float(ge), float(gq), float(b["margin"].min())


# twelve matches of a 600-match pair, four in each of the waves 0, 5 and 9 of k_map_tri's lanes (match i: wave i // 64), and
# what replaces which coordinate of which view's keypoint: every value meets both views and both coordinates
NONFINITE_AT = (3, 17, 40, 63, 321, 330, 350, 383, 577, 580, 590, 599)
NONFINITE = ((np.nan, 1, "x"), (np.inf, 1, "y"), (-np.inf, 2, "x"), (3e38, 2, "y"),
             (np.nan, 2, "y"), (np.inf, 2, "x"), (-np.inf, 1, "y"), (3e38, 1, "x"),
             (np.nan, 1, "y"), (np.inf, 2, "y"), (-np.inf, 1, "x"), (3e38, 2, "x"))


def nonfinite_pair():
    """(kq, kt, m, E1, E2, bad): a 600-match pair on rig 2 (match i pairs keypoint i with i) whose matches bad = NONFINITE_AT
    have one keypoint coordinate replaced as NONFINITE lists."""
    from aria_slam_amd import map_ref as M
    E1, E2 = views(2)
    kq, kt, m, _, _ = M.synth_scene(120, 600, E1, E2, depth=(1.0, 8.0))
    kq, kt = kq.copy(), kt.copy()
    for i, (value, view, coord) in zip(NONFINITE_AT, NONFINITE):
        (kq if view == 1 else kt)[coord][i] = value
    return kq, kt, m, E1, E2, np.array(NONFINITE_AT)
