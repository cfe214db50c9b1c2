"""NumPy fp64 restatement of the fundamental-matrix RANSAC stage (include/aria_orb_hip.h, "fundamental-matrix RANSAC";
kernels in aria_slam_amd/csrc/fund_ransac.hip): cv::findFundamentalMat(pts1, pts2, FM_RANSAC, 3.0, 0.99) as far as it can
be read from OpenCV 4.9.0's source, with the stage's fixed budget and sample hash. OpenCV is not available to this
project's tests, so this module is the specification; parity with a running OpenCV is not pinned.

- Small inputs: n < 15 gives no F (OpenCV's 7-point-only and LMeDS branches are not restated).
- Samples: pose_ref's hash, slots 0..6. A collinear sample (haveCollinearPoints on slot 6, both views) is invalid.
- run7Point: per-sample normalisation, elimination over columns 0..6, basis g1 (f7 = 1, f8 = 0), g2 (f7 = 0, f8 = 1), the
  cubic of f1 = g1 - g2, f2 = g2, closed-form real roots in ascending order, de-normalisation, F[8] = 1.
- Error: computeError in fp64 on the fp32 pixels, max of the two squared point-line distances, cast to float32 and
  compared with float32(thr^2); a zero line normal is an outlier.
- Winner: most inliers, ties to the lowest (h, k); at least 7 inliers; no refit.

The device scores in fp32 on conditioned points; its decisions equal this module's except for points whose error lies
within a relative 1e-3 of thr^2. verify_loop restates LoopClosureDetector::verifyGeometry + computeRelativePose
(src/legacy/LoopClosure.cpp:116-195) from this module and pose_ref.
"""
import numpy as np

from . import pose_ref
from ._lib import KP_DTYPE, MATCH_DTYPE

MIN_MATCHES = 15
MIN_INLIERS = 7
PIVOT_TOL = 1e-9
CUBIC_TOL = 1e-12
FLT_EPS = float(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)
TWO_PI_3 = 2.0 * 3.14159265358979323846 / 3.0
# computeRelativePose's hard-coded intrinsics (LoopClosure.cpp:171-174)
REFERENCE_LOOP_K = (700.0, 700.0, 320.0, 180.0)


def pixels(kp_query, kp_train, matches, query_is_first=True):
    """(n, 4) float32 pixel pairs (x1, y1, x2, y2) as the device stages them."""
    kq = np.asarray(kp_query).view(KP_DTYPE) if len(kp_query) else np.zeros(0, KP_DTYPE)
    kt = np.asarray(kp_train).view(KP_DTYPE) if len(kp_train) else np.zeros(0, KP_DTYPE)
    m = np.asarray(matches).view(MATCH_DTYPE) if len(matches) else np.zeros(0, MATCH_DTYPE)
    a, b = kq[m["query_idx"]], kt[m["train_idx"]]
    k1, k2 = (a, b) if query_is_first else (b, a)
    return np.stack([k1["x"], k1["y"], k2["x"], k2["y"]], axis=1).astype(np.float32).reshape(-1, 4)


def sample_indices(seed, pair, hypotheses, n):
    """(hypotheses, 7) sample indices: pose_ref's hash with k = 7; all -1 below 15 matches."""
    if n < MIN_MATCHES:
        return np.full((int(hypotheses), 7), -1, np.int64)
    return pose_ref.sample_indices(seed, pair, hypotheses, n, k=7)


def collinear(x, y):
    """haveCollinearPoints on (H, 7) coordinates: slot 6 against every pair of slots 0..5 (fp64, or the type given)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype != np.longdouble:
        x, y = x.astype(np.float64), y.astype(np.float64)
    col = np.zeros(x.shape[0], bool)
    for j in range(1, 6):
        dx1, dy1 = x[:, j] - x[:, 6], y[:, j] - y[:, 6]
        for k in range(j):
            dx2, dy2 = x[:, k] - x[:, 6], y[:, k] - y[:, 6]
            col |= np.abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPS * (np.abs(dx1) + np.abs(dy1) + np.abs(dx2) + np.abs(dy2))
    return col


def _normalisation(x, y):
    """run7Point's per-sample transform: centroid (mx, my) and scale sqrt(2) / mean distance; ok = mean >= FLT_EPSILON."""
    t = x.dtype.type(1.0) / x.dtype.type(7.0)
    mx, my = np.zeros(x.shape[0], x.dtype), np.zeros(x.shape[0], x.dtype)
    for i in range(7):
        mx = mx + x[:, i]
        my = my + y[:, i]
    mx, my = mx * t, my * t
    s = np.zeros(x.shape[0], x.dtype)
    for i in range(7):
        a, b = x[:, i] - mx, y[:, i] - my
        s = s + np.sqrt(a * a + b * b)
    s = s * t
    ok = s >= FLT_EPS
    return mx, my, np.sqrt(x.dtype.type(2.0)) / np.where(ok, s, 1.0), ok


def _rows(x1, y1, x2, y2):
    return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=-1)


def _wide(a):
    """fp64, unless the array already is np.longdouble (the extended run of solve7)."""
    a = np.asarray(a)
    return a if a.dtype == np.longdouble else a.astype(np.float64)


def cubic_coefficients(f1, f2):
    """run7Point's expansion of det(l f1 + f2) = c0 l^3 + c1 l^2 + c2 l + c3 for (H, 9) f1, f2. Returns (H, 4)."""
    f1 = [_wide(f1)[:, i] for i in range(9)]
    f2 = [_wide(f2)[:, i] for i in range(9)]
    t0 = f2[4] * f2[8] - f2[5] * f2[7]
    t1 = f2[3] * f2[8] - f2[5] * f2[6]
    t2 = f2[3] * f2[7] - f2[4] * f2[6]
    c3 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2
    c2 = (f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
          f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
          f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
          f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]))
    t0 = f1[4] * f1[8] - f1[5] * f1[7]
    t1 = f1[3] * f1[8] - f1[5] * f1[6]
    t2 = f1[3] * f1[7] - f1[4] * f1[6]
    c1 = (f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
          f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
          f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
          f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]))
    c0 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2
    return np.stack([c0, c1, c2, c3], axis=1)


def cubic_roots(c):
    """Real roots of c0 l^3 + c1 l^2 + c2 l + c3 (rows of (H, 4)), closed form as the device computes them: the
    trigonometric form when Q^3 - R^2 > 0 (three roots, ascending), Cardano otherwise (one). Returns (roots (H, 3), n (H,));
    n = 0 where |c0| <= 1e-12 max|c_i|."""
    c = _wide(c)
    T = c.dtype.type
    two_pi_3 = TWO_PI_3 if T is np.float64 else T(2) * np.arccos(T(-1)) / T(3)
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    ok = np.abs(c0) > CUBIC_TOL * np.abs(c).max(axis=1)
    with np.errstate(all="ignore"):
        d0 = np.where(ok, c0, 1.0)
        a1, a2, a3 = c1 / d0, c2 / d0, c3 / d0
        Q = (a1 * a1 - 3.0 * a2) * (T(1) / T(9))
        R = (a1 * (2.0 * a1 * a1 - 9.0 * a2) + 27.0 * a3) * (T(1) / T(54))
        disc = (a1 * a1 * (a2 * a2 - 4.0 * a1 * a3) + 2.0 * a2 * (9.0 * a1 * a3 - 2.0 * a2 * a2) - 27.0 * a3 * a3) * (T(1) / T(108))
        three = disc > 0.0
        theta = np.arccos(np.clip(R / np.sqrt(np.where(three, Q * Q * Q, 1.0)), -1.0, 1.0))
        sq, th, sh = -2.0 * np.sqrt(np.where(three, Q, 0.0)), theta * (T(1) / T(3)), a1 * (T(1) / T(3))
        r3 = np.sort(np.stack([sq * np.cos(th) - sh, sq * np.cos(th + two_pi_3) - sh, sq * np.cos(th - two_pi_3) - sh], 1), 1)
        e = np.cbrt(np.sqrt(np.where(three, 0.0, -disc)) + np.abs(R))
        e = np.where(R > 0.0, -e, e)
        r1 = (e + Q / e) - a1 * (T(1) / T(3))
    roots = np.where(three[:, None], r3, np.stack([r1, np.zeros_like(r1), np.zeros_like(r1)], 1))
    n = np.where(ok, np.where(three, 3, 1), 0)
    roots[n == 0] = 0.0
    return roots, n


def _models(f1, f2, roots, nroots, mx1, my1, s1, mx2, my2, s2):
    """run7Point's per-root model, de-normalised and scaled to F[8] = 1: (H, 3, 9), zero for k >= nroots."""
    H = f1.shape[0]
    dt = f1.dtype
    F = np.zeros((H, 3, 9), dt)
    T1x, T1y, T2x, T2y = -s1 * mx1, -s1 * my1, -s2 * mx2, -s2 * my2
    with np.errstate(all="ignore"):
        for k in range(3):
            lam, mu = roots[:, k].copy(), np.ones(H, dt)
            s = f1[:, 8] * lam + f2[:, 8]
            big = np.abs(s) > DBL_EPS
            mu = np.where(big, 1.0 / np.where(big, s, 1.0), mu)
            lam = np.where(big, lam * mu, lam)
            Fn = f1 * lam[:, None] + f2 * mu[:, None]
            Fn[:, 8] = np.where(big, 1.0, 0.0)
            M = np.empty((H, 9), dt)
            for j in range(3):
                M[:, j] = s2 * Fn[:, j]
                M[:, 3 + j] = s2 * Fn[:, 3 + j]
                M[:, 6 + j] = (T2x * Fn[:, j] + T2y * Fn[:, 3 + j]) + Fn[:, 6 + j]
            G = np.empty((H, 9), dt)
            for i in range(3):
                G[:, 3 * i] = M[:, 3 * i] * s1
                G[:, 3 * i + 1] = M[:, 3 * i + 1] * s1
                G[:, 3 * i + 2] = (M[:, 3 * i] * T1x + M[:, 3 * i + 1] * T1y) + M[:, 3 * i + 2]
            sc = np.abs(G[:, 8]) > FLT_EPS
            inv = 1.0 / np.where(sc, G[:, 8], 1.0)
            G = np.where(sc[:, None], G * inv[:, None], G)
            F[:, k] = np.where((k < nroots)[:, None], G, 0.0)
    return F


def solve7(samples, basis="elimination", dtype=np.float64):
    """run7Point on (H, 7, 4) pixel samples (fp32 values, fp64 arithmetic; dtype=np.longdouble is the extended run that the
    GPU tests measure the fp64 one against: every step is array arithmetic). Returns (F (H, 3, 9), n_models (H,)).
    basis="svd" takes the null space from the SVD as OpenCV does (f1, f2 = the last two right singular vectors) instead of
    the elimination basis -- the test of basis independence."""
    p = np.asarray(samples, dtype)
    H = p.shape[0]
    x1, y1, x2, y2 = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    ok = ~collinear(x1, y1) & ~collinear(x2, y2)
    mx1, my1, s1, ok1 = _normalisation(x1, y1)
    mx2, my2, s2, ok2 = _normalisation(x2, y2)
    ok &= ok1 & ok2
    A = _rows((x1 - mx1[:, None]) * s1[:, None], (y1 - my1[:, None]) * s1[:, None], (x2 - mx2[:, None]) * s2[:, None],
              (y2 - my2[:, None]) * s2[:, None])
    if basis == "svd":
        _u, _s, Vt = np.linalg.svd(A, full_matrices=True)
        f1, f2 = Vt[:, 7, :] - Vt[:, 8, :], Vt[:, 8, :].copy()
    else:
        ar = np.arange(H)
        amax = np.abs(A).reshape(H, -1).max(axis=1)
        A = A.copy()
        for c in range(7):
            col = np.abs(A[:, c:, c])
            piv = c + np.argmax(col, axis=1)
            ok &= col.max(axis=1) > PIVOT_TOL * amax
            rc = A[:, c, :].copy()
            A[:, c, :] = A[ar, piv, :]
            A[ar, piv, :] = rc
            inv = 1.0 / np.where(ok, A[:, c, c], 1.0)
            f = A[:, c + 1:, c] * inv[:, None]
            A[:, c + 1:, c + 1:] = A[:, c + 1:, c + 1:] - f[:, :, None] * A[:, c, None, c + 1:]
        g1, g2 = np.zeros((H, 9), dtype), np.zeros((H, 9), dtype)
        g1[:, 7], g2[:, 8] = 1.0, 1.0
        piv = np.where(ok[:, None], A[:, np.arange(7), np.arange(7)], 1.0)
        with np.errstate(all="ignore"):
            for c in range(6, -1, -1):
                u, v = np.zeros(H, dtype), np.zeros(H, dtype)
                for k in range(c + 1, 9):
                    u = u + A[:, c, k] * g1[:, k]
                    v = v + A[:, c, k] * g2[:, k]
                g1[:, c] = -u / piv[:, c]
                g2[:, c] = -v / piv[:, c]
        f1, f2 = g1 - g2, g2
    roots, nr = cubic_roots(cubic_coefficients(f1, f2))
    nr = np.where(ok, nr, 0)
    F = _models(f1, f2, roots, nr, mx1, my1, s1, mx2, my2, s2)
    fin = np.isfinite(F).all(axis=(1, 2))
    nr = np.where(fin, nr, 0)
    F[nr == 0] = 0.0
    return F, nr


def errors(F, pts):
    """computeError: (M, n) float32 max of the two squared point-line distances of every model in F (M, 9) on the (n, 4)
    pixel pairs, fp64 arithmetic; inf where a line normal is zero."""
    f = np.asarray(F, np.float64).reshape(-1, 9)
    p = np.asarray(pts, np.float64)
    x1, y1, x2, y2 = (p[:, i][None, :] for i in range(4))
    F_ = [f[:, k, None] for k in range(9)]
    a = F_[0] * x1 + F_[1] * y1 + F_[2]
    b = F_[3] * x1 + F_[4] * y1 + F_[5]
    c = F_[6] * x1 + F_[7] * y1 + F_[8]
    d2 = x2 * a + y2 * b + c
    n2 = a * a + b * b
    a = F_[0] * x2 + F_[3] * y2 + F_[6]
    b = F_[1] * x2 + F_[4] * y2 + F_[7]
    c = F_[2] * x2 + F_[5] * y2 + F_[8]
    d1 = x1 * a + y1 * b + c
    n1 = a * a + b * b
    with np.errstate(all="ignore"):
        e = np.maximum(d1 * d1 / np.where(n1 > 0, n1, 1.0), d2 * d2 / np.where(n2 > 0, n2, 1.0))
    e = np.where((n1 > 0) & (n2 > 0), e, np.inf)
    return e.astype(np.float32)


def threshold2(threshold_px=3.0):
    return np.float32(threshold_px * threshold_px)


def hypotheses(pts, seed=0, pair=0, n_hyp=1024, threshold_px=3.0):
    """What aria_fund_debug_hypotheses returns: (sample_idx (H, 7), n_models (H,), F (H, 3, 9), counts (H, 3); -1 = no model)."""
    n = len(pts)
    idx = sample_indices(seed, pair, n_hyp, n)
    F = np.zeros((n_hyp, 3, 9))
    nm = np.zeros(n_hyp, np.int64)
    counts = np.full((n_hyp, 3), -1, np.int64)
    have = (idx >= 0).all(axis=1)
    if have.any():
        Fv, nv = solve7(np.asarray(pts)[idx[have]])
        rows = np.flatnonzero(have)
        F[rows], nm[rows] = Fv, nv
    live = np.flatnonzero(nm > 0)
    if len(live):
        inl = errors(F[live].reshape(-1, 9), pts) <= threshold2(threshold_px)
        c = inl.sum(axis=1).reshape(-1, 3)
        k = np.arange(3)[None, :]
        counts[live] = np.where(k < nm[live, None], c, -1)
    return idx, nm, F, counts


def estimate_points(pts, seed=0, pair=0, n_hyp=1024, threshold_px=3.0, hyp=None):
    """The whole stage on (n, 4) pixel pairs: a dict with the fields of aria_fund_result and the mask. hyp: hypotheses()'s
    result for these arguments, if the caller has it already."""
    n = len(pts)
    res = dict(F=np.zeros((3, 3)), n_matches=n, n_inliers=0, n_models=0, best_hypothesis=-1, best_root=-1, valid=0,
               mask=np.zeros(n, np.uint8))
    if n < MIN_MATCHES:
        return res
    _idx, nm, F, counts = hyp if hyp is not None else hypotheses(pts, seed, pair, n_hyp, threshold_px)
    flat = counts.reshape(-1)
    best = int(np.argmax(flat))              # first maximum: ties to the lowest h, then k
    if flat[best] < MIN_INLIERS:
        return res
    h, k = divmod(best, 3)
    mask = (errors(F[h, k], pts)[0] <= threshold2(threshold_px)).astype(np.uint8)
    res.update(F=F[h, k].reshape(3, 3).copy(), n_inliers=int(mask.sum()), n_models=int(nm.sum()), best_hypothesis=h,
               best_root=k, valid=1, mask=mask)
    return res


def estimate(kp_query, kp_train, matches, query_is_first=True, seed=0, pair=0, n_hyp=1024, threshold_px=3.0):
    """aria_fund_estimate on the CPU."""
    return estimate_points(pixels(kp_query, kp_train, matches, query_is_first), seed, pair, n_hyp, threshold_px)


def pose_matrix(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def verify_loop(kp_query, kp_train, matches, min_matches, seed=0, pair=0, n_hyp=1024, pose_hyp=1024, K=REFERENCE_LOOP_K):
    """LoopClosureDetector::verifyGeometry + computeRelativePose (LoopClosure.cpp:116-195) restated: view 1 = the query
    keyframe. Returns dict(accepted, T (4x4 [R t; 0 1] or identity), matches (the F inliers, or empty), fund, pose)."""
    m = np.asarray(matches).view(MATCH_DTYPE) if len(matches) else np.zeros(0, MATCH_DTYPE)
    out = dict(accepted=False, T=np.eye(4), matches=np.zeros(0, MATCH_DTYPE), fund=None, pose=None)
    if len(m) < min_matches:
        return out
    f = estimate(kp_query, kp_train, m, True, seed, pair, n_hyp)
    out["fund"] = f
    if not f["valid"] or f["n_inliers"] < min_matches:
        return out
    inl = m[f["mask"] == 1]
    if len(inl) < 8:
        return out
    p = pose_ref.estimate(kp_query, kp_train, inl, True, seed, pair, pose_hyp, 1.0, 50.0, K)
    out["pose"] = p
    if not p["valid"] or p["n_pose_inliers"] < min_matches:
        return out
    out.update(accepted=True, T=pose_matrix(p["R"], p["t"]), matches=inl)
    return out


def synth_two_view(seed, n, R, t, outlier_frac=0.0, noise_px=0.5, K=REFERENCE_LOOP_K, width=640, height=360, depth=(2.0, 20.0)):
    """pose_ref.synth_two_view with the loop verifier's camera (700 / 700 / 320 / 180 at 640x360 by default)."""
    return pose_ref.synth_two_view(seed, n, R, t, outlier_frac, noise_px, K, width, height, depth)


def true_fundamental(R, t, K1=REFERENCE_LOOP_K, K2=None):
    """F = K2^-T [t]x R K1^-1 of X2 = R X1 + t, scaled to F[8] = 1 (x2^T F x1 = 0 in pixels)."""
    K2 = K1 if K2 is None else K2
    def kmat(k):
        return np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]])
    t = np.asarray(t, np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(kmat(K2)).T @ tx @ np.asarray(R) @ np.linalg.inv(kmat(K1))
    return F / F[2, 2]
