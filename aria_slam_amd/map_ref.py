"""NumPy restatement of the two-view triangulation stage and its point map (include/aria_orb_hip.h, "two-view triangulation
and point map"; kernels in csrc/map_triangulate.hip) -- the reference's Mapper::triangulate, filterOutliers and
filterByDistance (src/legacy/Mapper.cpp). Vectorised over points; every step follows the header's order of operations,
so kept positions agree with the device to rounding (the device's acos and summation order may differ in the last bits).

Also a scene generator with known extrinsics that returns the true world points, for the accuracy tests."""
import numpy as np

from ._lib import KP_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE

EUROC_K = (458.654, 457.296, 367.215, 248.375)
SVD_EPS = 10.0 * np.finfo(np.float64).eps
SVD_SWEEPS = 30
SVD_SWEEPS_EXT = 60                                      # sweep cap of an extended-precision run (the tests' yardstick)
W_EPS = 1e-10
MIN_MATCHES = 8
DEFAULTS = dict(min_depth=0.1, max_depth=50.0, min_parallax=1.0, max_reproj=2.0)

# rejection reasons of triangulate_points
KEPT, AT_INFINITY, DEPTH, PARALLAX, REPROJ = 0, 1, 2, 3, 4
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def as_extrinsics(T, dtype=np.float64):
    """[R | t] (3x4) from a 3x4 / 4x4 matrix or 12 row-major doubles."""
    T = np.asarray(T, dtype)
    return T.reshape(-1)[:12].reshape(3, 4) if T.size in (12, 16) else T[:3, :4]


def projection(K, E, dtype=np.float64):
    fx, fy, cx, cy = K
    E = as_extrinsics(E, dtype)
    return np.stack([fx * E[0] + cx * E[2], fy * E[1] + cy * E[2], E[2].copy()])


def dlt_null_vectors(A, dtype=np.float64):
    """A: (N, 4, 4) rows. One-sided Jacobi SVD per the header; returns (N, 4): the right singular vector of the smallest
    singular value. dtype: np.float64 is the stage's arithmetic (10 DBL_EPSILON, 30 sweeps); any other type runs the same
    steps with 10 of its own epsilon and a cap of 60 sweeps, so that the run is converged."""
    A = np.asarray(A, dtype)
    N = A.shape[0]
    eps, sweeps = (SVD_EPS, SVD_SWEEPS) if dtype == np.float64 else (10.0 * np.finfo(dtype).eps, SVD_SWEEPS_EXT)
    a = np.transpose(A, (0, 2, 1)).copy()                # a[:, c, :] = column c of A
    v = np.broadcast_to(np.eye(4, dtype=dtype), (N, 4, 4)).copy()     # v[:, c, :] = column c of V
    active = np.ones(N, bool)
    for _ in range(sweeps):
        if not active.any():
            break
        rot_any = np.zeros(N, bool)
        for i, j in PAIRS:
            ai, aj = a[:, i, :], a[:, j, :]
            alpha = ai[:, 0] * ai[:, 0] + ai[:, 1] * ai[:, 1] + ai[:, 2] * ai[:, 2] + ai[:, 3] * ai[:, 3]
            beta = aj[:, 0] * aj[:, 0] + aj[:, 1] * aj[:, 1] + aj[:, 2] * aj[:, 2] + aj[:, 3] * aj[:, 3]
            gamma = ai[:, 0] * aj[:, 0] + ai[:, 1] * aj[:, 1] + ai[:, 2] * aj[:, 2] + ai[:, 3] * aj[:, 3]
            rot = active & (np.abs(gamma) > eps * np.sqrt(alpha * beta))
            if not rot.any():
                continue
            rot_any |= rot
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                g = np.where(rot, gamma, 1.0)
                zeta = (beta - alpha) / (2.0 * g)
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
            c = np.where(rot, c, 1.0)[:, None]
            s = np.where(rot, s, 0.0)[:, None]
            x, y = ai.copy(), aj.copy()
            a[:, i, :] = np.where(rot[:, None], c * x - s * y, x)
            a[:, j, :] = np.where(rot[:, None], s * x + c * y, y)
            p, q = v[:, i, :].copy(), v[:, j, :].copy()
            v[:, i, :] = np.where(rot[:, None], c * p - s * q, p)
            v[:, j, :] = np.where(rot[:, None], s * p + c * q, q)
        active &= rot_any
    n2 = a[:, :, 0] * a[:, :, 0] + a[:, :, 1] * a[:, :, 1] + a[:, :, 2] * a[:, :, 2] + a[:, :, 3] * a[:, :, 3]
    k = np.argmin(n2, axis=1)                            # ties: lowest column
    return v[np.arange(N), k, :]


def triangulate_points(x1, x2, E1, E2, K=EUROC_K, min_depth=0.1, max_depth=50.0, min_parallax=1.0, max_reproj=2.0,
                       dtype=np.float64):
    """x1, x2: (N, 2) pixels (fp32 values); E1, E2: world-to-camera [R | t]. Returns (reason (N,) int, X (N, 3), err (N, 2)):
    reason KEPT or the first test that rejected the point. dtype: the arithmetic (see dlt_null_vectors); the inputs are
    the same fp32 pixels and fp64 extrinsics, intrinsics and thresholds in either."""
    x1 = np.asarray(x1, np.float32).astype(dtype).reshape(-1, 2)
    x2 = np.asarray(x2, np.float32).astype(dtype).reshape(-1, 2)
    E1, E2 = as_extrinsics(E1, dtype), as_extrinsics(E2, dtype)
    P1, P2 = projection(K, E1, dtype), projection(K, E2, dtype)
    N = len(x1)
    A = np.empty((N, 4, 4), dtype)
    A[:, 0] = x1[:, :1] * P1[2] - P1[0]
    A[:, 1] = x1[:, 1:] * P1[2] - P1[1]
    A[:, 2] = x2[:, :1] * P2[2] - P2[0]
    A[:, 3] = x2[:, 1:] * P2[2] - P2[1]
    Xh = dlt_null_vectors(A, dtype) if N else np.zeros((0, 4), dtype)
    reason = np.full(N, KEPT)
    inf = ~(np.abs(Xh[:, 3]) >= W_EPS)
    reason[inf] = AT_INFINITY
    w = np.where(inf, 1.0, Xh[:, 3])
    X = Xh[:, :3] / w[:, None]
    fx, fy, cx, cy = K
    with np.errstate(all="ignore"):
        c1 = X[:, 0:1] * E1[:, 0] + X[:, 1:2] * E1[:, 1] + X[:, 2:3] * E1[:, 2] + E1[:, 3]
        c2 = X[:, 0:1] * E2[:, 0] + X[:, 1:2] * E2[:, 1] + X[:, 2:3] * E2[:, 2] + E2[:, 3]
        depth_ok = (c1[:, 2] >= min_depth) & (c1[:, 2] <= max_depth) & (c2[:, 2] >= min_depth) & (c2[:, 2] <= max_depth)
        reason[(reason == KEPT) & ~depth_ok] = DEPTH
        C1 = -(E1[:, :3].T @ E1[:, 3])
        C2 = -(E2[:, :3].T @ E2[:, 3])
        r1, r2 = X - C1, X - C2
        n1 = np.sqrt(r1[:, 0] * r1[:, 0] + r1[:, 1] * r1[:, 1] + r1[:, 2] * r1[:, 2])
        n2 = np.sqrt(r2[:, 0] * r2[:, 0] + r2[:, 1] * r2[:, 1] + r2[:, 2] * r2[:, 2])
        cosp = (r1[:, 0] / n1) * (r2[:, 0] / n2) + (r1[:, 1] / n1) * (r2[:, 1] / n2) + (r1[:, 2] / n1) * (r2[:, 2] / n2)
        pi = np.pi if dtype == np.float64 else np.arccos(dtype(-1))
        par = np.arccos(np.minimum(1.0, np.abs(cosp))) * 180.0 / pi
        reason[(reason == KEPT) & ~(par >= min_parallax)] = PARALLAX
        e1x = fx * c1[:, 0] / c1[:, 2] + cx - x1[:, 0]
        e1y = fy * c1[:, 1] / c1[:, 2] + cy - x1[:, 1]
        e2x = fx * c2[:, 0] / c2[:, 2] + cx - x2[:, 0]
        e2y = fy * c2[:, 1] / c2[:, 2] + cy - x2[:, 1]
        err = np.stack([np.sqrt(e1x * e1x + e1y * e1y), np.sqrt(e2x * e2x + e2y * e2y)], 1)
        reason[(reason == KEPT) & ~((err[:, 0] <= max_reproj) & (err[:, 1] <= max_reproj))] = REPROJ
    return reason, X, err


def triangulate_pair(kp_query, kp_train, matches, pose1, pose2, image=None, mask=None, query_is_first=True, pair=0,
                     K=EUROC_K, **thresholds):
    """One pair: the kept points as MAP_POINT_DTYPE records in match order (id 0; Map.append numbers them).
    image: view 1's gray image (H, W) uint8 or None."""
    th = dict(DEFAULTS, **thresholds)
    m = np.asarray(matches).view(MATCH_DTYPE).reshape(-1)
    if len(m) < MIN_MATCHES:
        return np.zeros(0, MAP_POINT_DTYPE)
    kq, kt = np.asarray(kp_query).view(KP_DTYPE).reshape(-1), np.asarray(kp_train).view(KP_DTYPE).reshape(-1)
    qi, ti = m["query_idx"].astype(np.int64), m["train_idx"].astype(np.int64)
    if (qi < 0).any() or (qi >= len(kq)).any() or (ti < 0).any() or (ti >= len(kt)).any():
        raise ValueError("match index out of range")
    i1, i2 = (qi, ti) if query_is_first else (ti, qi)
    k1, k2 = (kq, kt) if query_is_first else (kt, kq)
    x1 = np.stack([k1["x"][i1], k1["y"][i1]], 1)
    x2 = np.stack([k2["x"][i2], k2["y"][i2]], 1)
    cand = np.ones(len(m), bool) if mask is None else (np.asarray(mask).reshape(-1)[:len(m)] != 0)
    reason, X, err = triangulate_points(x1, x2, pose1, pose2, K, th["min_depth"], th["max_depth"], th["min_parallax"],
                                        th["max_reproj"])
    keep = cand & (reason == KEPT)
    sel = np.flatnonzero(keep)
    out = np.zeros(len(sel), MAP_POINT_DTYPE)
    out["X"] = X[sel]
    out["quality"] = 1.0 / (err[sel, 0] + err[sel, 1] + 0.1)
    out["err"] = err[sel].astype(np.float32)
    out["pair"] = pair
    out["match"] = sel
    out["idx1"] = i1[sel]
    out["idx2"] = i2[sel]
    if image is None:
        out["gray"] = 127
    else:
        img = np.asarray(image, np.uint8)
        H, W = img.shape
        px = np.clip(np.trunc(x1[sel, 0]), 0, W - 1).astype(np.int64)
        py = np.clip(np.trunc(x1[sel, 1]), 0, H - 1).astype(np.int64)
        out["gray"] = img[py, px]
    return out


def filter_outliers(points):
    """Mapper::filterOutliers: no-op below 10 points; else remove |p - mean| > 3 sd (stable)."""
    if len(points) < 10:
        return points.copy()
    P = points["X"]
    mean = P.sum(axis=0) / len(P)
    d = P - mean
    sd = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sum() / len(P))
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return points[~(dist > 3.0 * sd)].copy()


def filter_distance(points, max_distance):
    """Mapper::filterByDistance: remove |p| > max_distance (stable)."""
    P = points["X"]
    return points[~(np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1] + P[:, 2] * P[:, 2]) > max_distance)].copy()


class Map:
    """The point map: records in append order, ids from a map-wide sequence."""

    def __init__(self):
        self.points = np.zeros(0, MAP_POINT_DTYPE)
        self.next_id = 0

    def append(self, pts):
        pts = pts.copy()
        pts["id"] = self.next_id + np.arange(len(pts), dtype=np.uint64)
        self.next_id += len(pts)
        self.points = np.concatenate([self.points, pts])
        return len(pts)

    def triangulate(self, *args, **kw):
        return self.append(triangulate_pair(*args, **kw))

    def filter_outliers(self):
        self.points = filter_outliers(self.points)

    def filter_distance(self, d):
        self.points = filter_distance(self.points, d)

    def clear(self):
        self.points = np.zeros(0, MAP_POINT_DTYPE)
        self.next_id = 0


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def extrinsics(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1)


def synth_scene(seed, n, E1, E2, outlier_frac=0.0, noise_px=0.5, K=EUROC_K, width=752, height=480, depth=(2.0, 20.0)):
    """Matched keypoints of n world points seen by two cameras with world-to-camera extrinsics E1, E2 (3x4).

    Returns (kp_query, kp_train, matches, X_world (n, 3), inlier_truth): query = view 1, match i pairs keypoint i with i;
    round(n * outlier_frac) matches (spread at random) pair view-1 points with random view-2 pixels."""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    E1, E2 = as_extrinsics(E1), as_extrinsics(E2)
    R1, t1 = E1[:, :3], E1[:, 3]
    p1, p2, Xw = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 3))
    k = 0
    for _ in range(1000):
        if k >= n:
            break
        u = rng.uniform(0, width, 4 * n)
        v = rng.uniform(0, height, 4 * n)
        z = rng.uniform(depth[0], depth[1], 4 * n)
        Xc1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
        X = (Xc1 - t1) @ R1                               # R1^T (Xc1 - t1), row-wise
        Xc2 = X @ E2[:, :3].T + E2[:, 3]
        keep = Xc2[:, 2] > 0.5
        zs = np.where(keep, Xc2[:, 2], 1)
        u2 = fx * Xc2[:, 0] / zs + cx
        v2 = fy * Xc2[:, 1] / zs + cy
        keep &= (u2 >= 0) & (u2 < width) & (v2 >= 0) & (v2 < height)
        sel = np.flatnonzero(keep)[: n - k]
        p1[k:k + len(sel)] = np.stack([u[sel], v[sel]], 1)
        p2[k:k + len(sel)] = np.stack([u2[sel], v2[sel]], 1)
        Xw[k:k + len(sel)] = X[sel]
        k += len(sel)
    if k < n:
        raise ValueError("synth_scene: the two views share too little of the scene")
    p1 += rng.normal(0, noise_px, p1.shape) if noise_px > 0 else 0
    p2 += rng.normal(0, noise_px, p2.shape) if noise_px > 0 else 0
    n_out = int(round(n * outlier_frac))
    truth = np.ones(n, bool)
    out_idx = rng.permutation(n)[:n_out]
    truth[out_idx] = False
    p2[out_idx] = np.stack([rng.uniform(0, width, n_out), rng.uniform(0, height, n_out)], 1)
    kq, kt = np.zeros(n, KP_DTYPE), np.zeros(n, KP_DTYPE)
    kq["x"], kq["y"] = p1[:, 0], p1[:, 1]
    kt["x"], kt["y"] = p2[:, 0], p2[:, 1]
    for kk in (kq, kt):
        kk["size"] = 31.0
        kk["response"] = 1.0
    m = np.zeros(n, MATCH_DTYPE)
    m["query_idx"] = np.arange(n)
    m["train_idx"] = np.arange(n)
    return kq, kt, m, Xw, truth
