"""NumPy restatement of the loop alignment stage (include/aria_orb_hip.h, "loop alignment"; kernels in
aria_slam_amd/csrc/sim3_align.hip): the similarity X2 = s R X1 + t between the landmarks two keyframes own, by RANSAC over
three-point closed forms, two-sided fp32 reprojection scoring and a Gauss-Newton refinement over (w, v, sigma).

The reference project has no code for this step, so this module is the definition the device is held to
(tests/test_gpu_sim3.py over the table of tests/sim3_cases.py). Parity with ORB-SLAM's Sim3Solver is not claimed.

What runs in which precision: the closed form in fp64 with + - * / and sqrt alone and in the device's order of operations
(the Jacobi sweeps included, so the hypotheses agree bit for bit where the compiler contracts nothing); every inlier test in
fp32 in the device's order; the refinement and the outputs in fp64 -- or, with estimate(dtype=np.longdouble), in extended
precision, the yardstick that rounding is measured against (tools/sim3_gap.py). The hypotheses and every inlier test are the
same in both runs.

The scale step. The refinement's update is R <- Exp(w) R, t <- E(sigma) (Exp(w) t) + v, s <- E(sigma) s, where E is NOT libm's
exp but the fixed polynomial exp_series: the degree-12 Taylor sum in Horner form, + * / only, so host and device compute the
same bits. E(0) = 1 and E'(0) = 1 are all the Gauss-Newton step needs; at the fixed point sigma = 0 and the polynomial's
error does not enter the result. A step that takes s outside [min_scale, max_scale] (a negative polynomial value included)
ends the refinement with the last good model."""
import numpy as np

from ._lib import KP_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE, SIM3_CORR_DTYPE
from . import pose_ref as P
from .pnp_ref import cholesky_solve, exp_so3
from .pose_ref import EUROC_K

AREA_TOL = 1e-12      # |(Xb - Xa) x (Xc - Xa)|^2 <= tol * max(side^2)^2 in either frame: collinear or coincident sample
RANGE = 1e15          # a scoring value or |t| beyond this never scores: squares stay finite in fp32
MIN_CORR = 3          # a sample
MIN_REFINE = 4        # the least inliers a refinement starts from
STEP_TOL = 1e-12
JACOBI_SWEEPS = 10
EXP_TERMS = 12


def sample_indices(seed, pair, hypotheses, n):
    """(hypotheses, 3) sample indices: the pose stage's hash with 3 slots."""
    return P.sample_indices(seed, pair, hypotheses, n, k=3)


def threshold2(threshold_px=3.0, K=EUROC_K):
    t = threshold_px / ((K[0] + K[1]) * 0.5)
    return np.float32(t * t)


def as_corr(corr):
    c = np.ascontiguousarray(corr)
    if c.dtype != SIM3_CORR_DTYPE:
        c = c.view(SIM3_CORR_DTYPE)
    return c.reshape(-1)


def stage(corr, K=EUROC_K):
    """What k_sim3_stage leaves: X1, X2 (n, 3) fp64, x1, x2 (n, 2) fp64 normalised pixels, their fp32 roundings X1_32, X2_32,
    x1_32, x2_32 (all NaN for a correspondence with a value beyond RANGE), and `finite`: False when any X or pixel of the
    pair is not finite -- the pair is then refused before any arithmetic (valid = 0, a deferred error)."""
    c = as_corr(corr)
    fx, fy, cx, cy = K
    n = len(c)
    X1 = c["X1"].astype(np.float64).reshape(n, 3)
    X2 = c["X2"].astype(np.float64).reshape(n, 3)
    px = np.stack([c["u1"], c["v1"], c["u2"], c["v2"]], axis=1).astype(np.float64).reshape(n, 4)
    finite = bool(np.isfinite(X1).all() and np.isfinite(X2).all() and np.isfinite(px).all())
    with np.errstate(all="ignore"):
        x1 = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy], axis=1)
        x2 = np.stack([(px[:, 2] - cx) / fx, (px[:, 3] - cy) / fy], axis=1)
        f = [a.astype(np.float32) for a in (X1, X2, x1, x2)]
        lim = np.float32(RANGE)
        bad = ~np.logical_and.reduce([(np.abs(a) <= lim).all(axis=1) for a in f])
    for a in f:
        a[bad] = np.nan
    return dict(X1=X1, X2=X2, x1=x1, x2=x2, X1_32=f[0], X2_32=f[1], x1_32=f[2], x2_32=f[3], finite=finite)


# ---- the closed form ----------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _degenerate(Xa, Xb, Xc):
    e1, e2, e3 = _sub(Xb, Xa), _sub(Xc, Xa), _sub(Xc, Xb)
    n = _cross(e1, e2)
    amax = np.maximum(np.maximum(_dot(e1, e1), _dot(e2, e2)), _dot(e3, e3))
    return ~(_dot(n, n) > AREA_TOL * (amax * amax))


def jacobi3(G, dtype=np.float64):
    """The device's jacobi3 on (H, 3, 3) symmetric matrices, in `dtype`: JACOBI_SWEEPS cyclic sweeps over (0,1), (0,2), (1,2), a rotation
    skipped where its off-diagonal entry is exactly 0. Returns (eigenvalues (H, 3) = the diagonal, V (H, 3, 3), columns)."""
    A = np.array(G, dtype)
    H = A.shape[0]
    V = np.zeros((H, 3, 3), dtype)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _sweep in range(JACOBI_SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[:, p, q].copy()
                go = apq != 0.0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(go, apq, 1.0))
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                B = A.copy()
                for k in range(3):
                    akp, akq = A[:, k, p], A[:, k, q]
                    B[:, k, p], B[:, k, q] = c * akp - s * akq, s * akp + c * akq
                C = B.copy()
                for k in range(3):
                    apk, aqk = B[:, p, k], B[:, q, k]
                    C[:, p, k], C[:, q, k] = c * apk - s * aqk, s * apk + c * aqk
                C[:, p, q] = 0.0
                C[:, q, p] = 0.0
                W = V.copy()
                for k in range(3):
                    vkp, vkq = V[:, k, p], V[:, k, q]
                    W[:, k, p], W[:, k, q] = c * vkp - s * vkq, s * vkp + c * vkq
                A = np.where(go[:, None, None], C, A)
                V = np.where(go[:, None, None], W, V)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def solve_minimal(X1, X2, fix_scale=0, min_scale=0.05, max_scale=20.0, dtype=np.float64):
    """The three-point closed form on (H, 3, 3) point triples (sample slot, coordinate) of the two frames, in `dtype` (the
    device: fp64) and in the device's order of operations. Returns (R (H, 3, 3), t (H, 3), s (H,), valid (H,)): X2 = s R X1 + t."""
    X1 = np.asarray(X1, dtype)
    X2 = np.asarray(X2, dtype)
    H = X1.shape[0]
    with np.errstate(all="ignore"):
        A = [tuple(X1[:, i, k] for k in range(3)) for i in range(3)]
        B = [tuple(X2[:, i, k] for k in range(3)) for i in range(3)]
        ok = ~_degenerate(*A) & ~_degenerate(*B)
        c1 = tuple(((A[0][k] + A[1][k]) + A[2][k]) / 3.0 for k in range(3))
        c2 = tuple(((B[0][k] + B[1][k]) + B[2][k]) / 3.0 for k in range(3))
        q = [_sub(A[i], c1) for i in range(3)]
        p = [_sub(B[i], c2) for i in range(3)]
        M = [[(p[0][r] * q[0][c] + p[1][r] * q[1][c]) + p[2][r] * q[2][c] for c in range(3)] for r in range(3)]
        G = np.zeros((H, 3, 3), dtype)
        for r in range(3):
            for c in range(3):
                G[:, r, c] = (M[0][r] * M[0][c] + M[1][r] * M[1][c]) + M[2][r] * M[2][c]
        lam, V = jacobi3(G, dtype)
        l = [lam[:, 0], lam[:, 1], lam[:, 2]]
        col = [[V[:, 0, j], V[:, 1, j], V[:, 2, j]] for j in range(3)]

        def swap_if(sw, i, j):
            l[i], l[j] = np.where(sw, l[j], l[i]), np.where(sw, l[i], l[j])
            for k in range(3):
                col[i][k], col[j][k] = np.where(sw, col[j][k], col[i][k]), np.where(sw, col[i][k], col[j][k])

        swap_if(l[1] > l[0], 0, 1)
        swap_if(l[2] > l[1], 1, 2)
        swap_if(l[1] > l[0], 0, 1)
        sig1, sig2 = np.sqrt(np.maximum(l[0], 0.0)), np.sqrt(np.maximum(l[1], 0.0))
        v1, v2 = col[0], col[1]
        u1 = tuple(((M[r][0] * v1[0] + M[r][1] * v1[1]) + M[r][2] * v1[2]) / sig1 for r in range(3))
        u2 = tuple(((M[r][0] * v2[0] + M[r][1] * v2[1]) + M[r][2] * v2[2]) / sig2 for r in range(3))
        u3, v3 = _cross(u1, u2), _cross(v1, v2)
        R = np.zeros((H, 3, 3), dtype)
        for r in range(3):
            for c in range(3):
                R[:, r, c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c]
        if fix_scale:
            s = np.ones(H, dtype)
        else:
            den = (_dot(q[0], q[0]) + _dot(q[1], q[1])) + _dot(q[2], q[2])
            s = (sig1 + sig2) / den
            ok &= (s >= min_scale) & (s <= max_scale)
        t = np.stack([c2[k] - s * ((R[:, k, 0] * c1[0] + R[:, k, 1] * c1[1]) + R[:, k, 2] * c1[2]) for k in range(3)], axis=1)
        ok &= np.isfinite(R.astype(np.float64)).all(axis=(1, 2)) & np.isfinite(t.astype(np.float64)).all(axis=1)
        ok &= np.isfinite(s.astype(np.float64))
        ok &= (np.abs(t) <= RANGE).all(axis=1)
    R[~ok] = 0.0
    t[~ok] = 0.0
    s = np.where(ok, s, 0.0)
    return R, t, s, ok


# ---- scoring ------------------------------------------------------------------------------------------------------------------
def scored_model(R, t, s):
    """(R32 (H, 9), t32 (H, 3), s32 (H,), ok): the model rounded to fp32 as it is scored; ok = finite and |t| <= RANGE."""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    s = np.asarray(s, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        R32, t32, s32 = R.astype(np.float32), t.astype(np.float32), s.astype(np.float32)
        ok = np.isfinite(R32).all(axis=1) & (np.abs(t32) <= np.float32(RANGE)).all(axis=1) & np.isfinite(s32)
    R32[~ok] = 0
    t32[~ok] = 0
    s32[~ok] = 0
    return R32, t32, s32, ok


def _project32(R32, t32, s32, st, dt=np.float32):
    """(Y2, Y1): the two transfers in the device's association, computed in `dt` from the fp32 values.
    Y2[k] = s ((r[3k] X + r[3k+1] Y) + r[3k+2] Z) + t[k] on X1; Y1[k] = (r[k] d0 + r[3+k] d1) + r[6+k] d2, d = X2 - t."""
    R = np.asarray(R32, np.float32).reshape(-1, 9).astype(dt)
    t = np.asarray(t32, np.float32).reshape(-1, 3).astype(dt)
    s = np.asarray(s32, np.float32).reshape(-1).astype(dt)
    A, B = st["X1_32"].astype(dt), st["X2_32"].astype(dt)
    with np.errstate(all="ignore"):
        Y2 = [s[:, None] * ((R[:, 3 * k, None] * A[None, :, 0] + R[:, 3 * k + 1, None] * A[None, :, 1])
                            + R[:, 3 * k + 2, None] * A[None, :, 2]) + t[:, k, None] for k in range(3)]
        d = [B[None, :, k] - t[:, k, None] for k in range(3)]
        Y1 = [(R[:, k, None] * d[0] + R[:, 3 + k, None] * d[1]) + R[:, 6 + k, None] * d[2] for k in range(3)]
    return Y2, Y1


def inliers32(R32, t32, s32, st, thr2):
    """(H, n) bool, the device's two-sided test in fp32 and its order: for Y2 against x2 and Y1 against x1,
    Y.z > 0 and (Y.x - x Y.z)^2 + (Y.y - y Y.z)^2 <= thr2 Y.z^2."""
    Y2, Y1 = _project32(R32, t32, s32, st)
    x1, x2 = st["x1_32"], st["x2_32"]
    thr2 = np.float32(thr2)
    with np.errstate(all="ignore"):
        ex, ey = Y2[0] - x2[None, :, 0] * Y2[2], Y2[1] - x2[None, :, 1] * Y2[2]
        in2 = (Y2[2] > 0) & (ex * ex + ey * ey <= thr2 * (Y2[2] * Y2[2]))
        ex, ey = Y1[0] - x1[None, :, 0] * Y1[2], Y1[1] - x1[None, :, 1] * Y1[2]
        in1 = (Y1[2] > 0) & (ex * ex + ey * ey <= thr2 * (Y1[2] * Y1[2]))
    return in2 & in1


def error_ratio(R32, t32, s32, st, thr2):
    """(H, n) fp64: the larger of the two directions' squared error over thr2 z^2 (inf where a z <= 0 or a value is not
    finite) -- 1 at the threshold, an inlier at or below it; the tests' band."""
    Y2, Y1 = _project32(R32, t32, s32, st, np.float64)
    x1, x2 = st["x1_32"].astype(np.float64), st["x2_32"].astype(np.float64)
    out = None
    with np.errstate(all="ignore"):
        for Y, x in ((Y2, x2), (Y1, x1)):
            ex, ey = Y[0] - x[None, :, 0] * Y[2], Y[1] - x[None, :, 1] * Y[2]
            r = (ex * ex + ey * ey) / (float(thr2) * Y[2] * Y[2])
            r = np.where((Y[2] > 0) & np.isfinite(r), r, np.inf)
            out = r if out is None else np.maximum(out, r)
    return out


def hypotheses(corr, seed=0, pair=0, n_hyp=1024, threshold_px=3.0, K=EUROC_K, fix_scale=0, min_scale=0.05, max_scale=20.0,
               staged=None, models=None):
    """What aria_sim3_debug_hypotheses returns: (sample_idx (H, 3), R (H, 9) fp32, t (H, 3) fp32, s (H,) fp32, counts (H,),
    -1 = invalid). `models`, a list, receives the fp64 closed forms (R (H, 3, 3), t (H, 3), s (H,))."""
    st = staged if staged is not None else stage(corr, K)
    n = len(st["X1"])
    idx = sample_indices(seed, pair, n_hyp, n)
    valid = (idx >= 0).all(axis=1)
    if not st["finite"]:
        valid[:] = False
    R64, t64, s64 = np.zeros((n_hyp, 3, 3)), np.zeros((n_hyp, 3)), np.zeros(n_hyp)
    R32, t32, s32 = np.zeros((n_hyp, 9), np.float32), np.zeros((n_hyp, 3), np.float32), np.zeros(n_hyp, np.float32)
    counts = np.full(n_hyp, -1, np.int64)
    if valid.any():
        rows = np.flatnonzero(valid)
        R, t, s, ok = solve_minimal(st["X1"][idx[rows]], st["X2"][idx[rows]], fix_scale, min_scale, max_scale)
        r32, tt32, ss32, ok2 = scored_model(R, t, s)
        ok &= ok2
        R64[rows[ok]], t64[rows[ok]], s64[rows[ok]] = R[ok], t[ok], s[ok]
        R32[rows[ok]], t32[rows[ok]], s32[rows[ok]] = r32[ok], tt32[ok], ss32[ok]
        valid[rows[~ok]] = False
    if valid.any():
        thr2 = threshold2(threshold_px, K)
        live = np.flatnonzero(valid)
        for a in range(0, len(live), 256):
            sel = live[a:a + 256]
            counts[sel] = inliers32(R32[sel], t32[sel], s32[sel], st, thr2).sum(axis=1)
    if models is not None:
        models.append((R64, t64, s64))
    return idx, R32, t32, s32, counts


# ---- refinement ---------------------------------------------------------------------------------------------------------------
def exp_series(x, dtype=np.float64):
    """E(x): the degree-EXP_TERMS Taylor sum of exp in Horner form, 1 + x (1 + x/2 (1 + x/3 ( ... (1 + x/12)))), + * / only."""
    x = dtype(x)
    acc = dtype(1)
    for k in range(EXP_TERMS, 0, -1):
        acc = dtype(1) + (x / dtype(k)) * acc
    return acc


def residuals(R, t, s, X1, X2, x1, x2):
    """(n, 4) normalised reprojection residuals: Y2 = s R X1 + t against x2, then Y1 = R^T (X2 - t) against x1."""
    Y2 = s * (X1 @ R.T) + t
    Y1 = (X2 - t) @ R
    return np.stack([Y2[:, 0] / Y2[:, 2] - x2[:, 0], Y2[:, 1] / Y2[:, 2] - x2[:, 1],
                     Y1[:, 0] / Y1[:, 2] - x1[:, 0], Y1[:, 1] / Y1[:, 2] - x1[:, 1]], axis=1)


def gn_jacobian(R, t, s, X1, X2):
    """(n, 4, 7): d residual / d (w, v, sigma) of the left update R <- Exp(w) R, t <- E(sigma) Exp(w) t + v, s <- E(sigma) s
    at 0. To first order Y2 moves by w x Y2 + v + sigma Y2 (the last along the ray: no image motion) and Y1 by
    R^T (X2 x w - v - sigma t)."""
    dt = R.dtype
    n = len(X1)
    Y2 = s * (X1 @ R.T) + t
    Y1 = (X2 - t) @ R
    J = np.zeros((n, 4, 7), dt)
    iz = 1 / Y2[:, 2]
    px, py = Y2[:, 0] * iz, Y2[:, 1] * iz
    # d Y2 = -[Y2]x w + v: the absolute pose stage's rows with Xc = Y2
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2] = -(px * py), 1 + px * px, -py
    J[:, 0, 3], J[:, 0, 5] = iz, -(px * iz)
    J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = -(1 + py * py), px * py, px
    J[:, 1, 4], J[:, 1, 5] = iz, -(py * iz)
    iz = 1 / Y1[:, 2]
    px, py = Y1[:, 0] * iz, Y1[:, 1] * iz
    # d Y1 = R^T ([X2]x w - v - sigma t): D = R^T [X2]x (3x3), then the projection's rows (iz, 0, -px iz), (0, iz, -py iz)
    z = np.zeros(n, dt)
    Kx = np.stack([np.stack([z, -X2[:, 2], X2[:, 1]], axis=1), np.stack([X2[:, 2], z, -X2[:, 0]], axis=1),
                   np.stack([-X2[:, 1], X2[:, 0], z], axis=1)], axis=1)                       # (n, 3, 3) [X2]x
    D = np.einsum("ji,njk->nik", R, Kx)                                                       # R^T [X2]x
    Rt_t = R.T @ t
    for k in range(3):
        J[:, 2, k] = iz * D[:, 0, k] - (px * iz) * D[:, 2, k]
        J[:, 3, k] = iz * D[:, 1, k] - (py * iz) * D[:, 2, k]
        J[:, 2, 3 + k] = -(iz * R[k, 0] - (px * iz) * R[k, 2])
        J[:, 3, 3 + k] = -(iz * R[k, 1] - (py * iz) * R[k, 2])
    J[:, 2, 6] = -(iz * Rt_t[0] - (px * iz) * Rt_t[2])
    J[:, 3, 6] = -(iz * Rt_t[1] - (py * iz) * Rt_t[2])
    return J


def refine(R, t, s, X1, X2, x1, x2, iters, fix_scale=0, min_scale=0.05, max_scale=20.0, dtype=np.float64):
    """Up to `iters` Gauss-Newton steps over a fixed correspondence set. Returns (R, t, s, steps taken)."""
    R, t, s = np.asarray(R, dtype), np.asarray(t, dtype), dtype(s)
    npar = 6 if fix_scale else 7
    done = 0
    for _ in range(iters):
        with np.errstate(all="ignore"):
            J = gn_jacobian(R, t, s, X1, X2)[:, :, :npar].reshape(-1, npar)
            r = residuals(R, t, s, X1, X2, x1, x2).reshape(-1)
            A, b = J.T @ J, J.T @ r
        if not (np.isfinite(A.astype(np.float64)).all() and np.isfinite(b.astype(np.float64)).all()):
            break
        delta = cholesky_solve(A, -b)
        if delta is None:
            break
        es = dtype(1) if fix_scale else exp_series(delta[6], dtype)
        sn = es * s
        if not fix_scale and not (sn >= dtype(min_scale) and sn <= dtype(max_scale)):
            break
        E = exp_so3(delta[:3], dtype)
        R, t, s = E @ R, es * (E @ t) + delta[3:6], sn
        done += 1
        if np.sqrt((delta * delta).sum()) <= dtype(STEP_TOL):
            break
    return R, t, s, done


def _invalid(n):
    return dict(R=np.eye(3), t=np.zeros(3), s=1.0, rms_px=0.0, n_corr=n, n_inliers=0, best_hypothesis=-1, iterations=0,
                refined=0, valid=0, mask=np.zeros(n, np.uint8), winner=None, refit=None, n_winner=0, n_refit=0)


def estimate(corr, seed=0, pair=0, n_hyp=1024, threshold_px=3.0, refine_iters=5, K=EUROC_K, fix_scale=0, min_scale=0.05,
             max_scale=20.0, dtype=np.float64, hyp=None, models=None, staged=None):
    """aria_sim3_estimate on the CPU: a dict of the aria_sim3_result fields and the mask, plus what the tests need to judge a
    case: winner / refit ((R32, t32, s32) of the winning model as scored and of the refined model as rescored, whether or not
    it was kept; refit is None without a refinement) and n_winner / n_refit. dtype=np.longdouble: the refinement and the
    outputs in extended precision. hyp / models: what hypotheses() returned and appended, to save the work."""
    st = staged if staged is not None else stage(corr, K)
    n = len(st["X1"])
    if not st["finite"]:
        return _invalid(0)                     # refused before it is read: the record says n_corr = 0
    res = _invalid(n)
    if n < MIN_CORR:
        return res
    if hyp is None:
        models = []
        hyp = hypotheses(corr, seed, pair, n_hyp, threshold_px, K, fix_scale, min_scale, max_scale, st, models)
        models = models[0]
    _idx, R32, t32, s32, counts = hyp
    best = int(np.argmax(counts))
    if counts[best] < 0:
        return res
    dt = dtype
    thr2 = threshold2(threshold_px, K)
    inl = inliers32(R32[best], t32[best], s32[best], st, thr2)[0]
    n_win = int(inl.sum())
    # the kept model starts as the winner's closed form (what was scored is its fp32 rounding); the extended run solves the
    # winner's sample again in extended precision, so that GAP holds the closed form's rounding too
    Rk, tk, sk = models[0][best].astype(dt), models[1][best].astype(dt), dt(models[2][best])
    if dt is not np.float64:
        pick = _idx[best][None]
        Re, te, se, _ok = solve_minimal(st["X1"][pick], st["X2"][pick], fix_scale, min_scale, max_scale, dt)
        Rk, tk, sk = Re[0], te[0], se[0]
    X1, X2, x1, x2 = (st[k].astype(dt) for k in ("X1", "X2", "x1", "x2"))
    final_inl, refined, iterations, refit, n_refit = inl, 0, 0, None, 0
    if n_win >= MIN_REFINE and refine_iters > 0:
        Rr, tr, sr, iterations = refine(Rk, tk, sk, X1[inl], X2[inl], x1[inl], x2[inl], refine_iters, fix_scale, min_scale,
                                        max_scale, dt)
        if iterations:
            r32, tt32, ss32, good = scored_model(Rr.astype(np.float64), tr.astype(np.float64), np.float64(sr))
            if good[0]:
                inl_r = inliers32(r32, tt32, ss32, st, thr2)[0]
                refit, n_refit = (r32[0], tt32[0], ss32[0]), int(inl_r.sum())
                if n_refit >= n_win:
                    Rk, tk, sk, final_inl, refined = Rr, tr, sr, inl_r, 1
    n_in = int(final_inl.sum())
    rms = dt(0)
    with np.errstate(all="ignore"):
        if n_in:
            r = residuals(Rk, tk, sk, X1[final_inl], X2[final_inl], x1[final_inl], x2[final_inl])
            rms = np.sqrt((r * r).sum() / dt(2 * n_in)) * dt((K[0] + K[1]) * 0.5)
    if not (np.isfinite(Rk.astype(np.float64)).all() and np.isfinite(tk.astype(np.float64)).all() and np.isfinite(float(sk))
            and np.isfinite(float(rms))):
        return res
    res.update(R=Rk, t=tk, s=sk, rms_px=rms, n_inliers=n_in, best_hypothesis=best, iterations=iterations, refined=refined,
               valid=1, mask=final_inl.astype(np.uint8), winner=(R32[best], t32[best], s32[best]), refit=refit, n_winner=n_win,
               n_refit=n_refit)
    return res


# ---- the join -----------------------------------------------------------------------------------------------------------------
def associate(points, anchor1, anchor2, view1, view2, pose1, pose2, kp1, kp2, matches, kp_stride=None):
    """aria_sim3_associate_batch_device for one pair on the CPU: (corr, corr_match). Keyframe j owns the map points with
    pair == anchor_j, looked up by their idx{view_j}; match m (query = keyframe 1, train = keyframe 2) yields a correspondence
    when both sides have such a point -- of several the one at the lowest arena position, per side. X_j = R_j X + t_j with the
    12-double world-to-camera rows pose_j, each component ((r0 X + r1 Y) + r2 Z) + t; the pixels are the keypoints'. Match
    order is kept. kp_stride: arena indices outside [0, kp_stride) own nothing (default: no upper bound)."""
    pts = np.asarray(points).view(MAP_POINT_DTYPE).reshape(-1)
    k1 = np.asarray(kp1).view(KP_DTYPE).reshape(-1)
    k2 = np.asarray(kp2).view(KP_DTYPE).reshape(-1)
    m = np.asarray(matches).view(MATCH_DTYPE).reshape(-1)
    tables = []
    for anchor, view in ((anchor1, view1), (anchor2, view2)):
        key = pts["idx1"] if view == 1 else pts["idx2"]
        first = {}
        for pos in np.flatnonzero(pts["pair"] == anchor):
            k = int(key[pos])
            if k < 0 or (kp_stride is not None and k >= kp_stride):
                continue
            first.setdefault(k, int(pos))
        tables.append(first)
    poses = [np.asarray(p, np.float64).reshape(3, 4) for p in (pose1, pose2)]

    def move(T, X):
        return [((T[k, 0] * X[0] + T[k, 1] * X[1]) + T[k, 2] * X[2]) + T[k, 3] for k in range(3)]

    corr, back = [], []
    for i, a in enumerate(m):
        p1, p2 = tables[0].get(int(a["query_idx"])), tables[1].get(int(a["train_idx"]))
        if p1 is None or p2 is None:
            continue
        c = np.zeros(1, SIM3_CORR_DTYPE)
        c["X1"] = move(poses[0], pts["X"][p1])
        c["X2"] = move(poses[1], pts["X"][p2])
        c["u1"], c["v1"] = k1["x"][a["query_idx"]], k1["y"][a["query_idx"]]
        c["u2"], c["v2"] = k2["x"][a["train_idx"]], k2["y"][a["train_idx"]]
        corr.append(c)
        back.append(i)
    return (np.concatenate(corr) if corr else np.zeros(0, SIM3_CORR_DTYPE)), np.asarray(back, np.int32)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def synth_sim3(scene, n, R, t, s, outliers=0.0, noise_px=0.5, K=EUROC_K, w=752, h=480, depth_noise=0.0, shape="cloud"):
    """Two cameras seeing one cloud: X1 are the points in camera 1's coordinates in map 1's units, X2 = s R X1 + t the same
    points in camera 2's coordinates in map 2's units (map 1 is map 2 scaled by 1 / s), each projected into its own camera.
    Gaussian noise of noise_px on the four pixels; each landmark then moved along its own ray by the relative depth_noise
    (a triangulated point is uncertain along the ray, certain in the image). The first round(n * outliers) of a random
    permutation are outliers: their camera-2 sides are exchanged among themselves (random re-pairings).
    shape: "cloud" (depths 2-20 in front of camera 1, kept where camera 2 sees them too), "planar" (one tilted plane) or
    "line" (one 3-D line: every sample is collinear).

    Returns (corr (SIM3_CORR_DTYPE), inlier_truth (bool))."""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(scene)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    X1 = np.zeros((0, 3))
    while len(X1) < n:
        m = 4 * n + 16
        if shape == "line":
            a = rng.uniform(-2.0, 2.0, m)
            d = np.array([1.0, 0.3, 0.5]) / np.linalg.norm([1.0, 0.3, 0.5])
            X = np.array([0.0, 0.0, 8.0]) + a[:, None] * d
        else:
            u, v = rng.uniform(0, w, m), rng.uniform(0, h, m)
            xn, yn = (u - cx) / fx, (v - cy) / fy
            z = 6.0 / (1.0 - 0.3 * xn - 0.2 * yn) if shape == "planar" else rng.uniform(2.0, 20.0, m)
            X = np.stack([xn * z, yn * z, z], axis=1)
        Y = s * (X @ R.T) + t
        keep = Y[:, 2] > 0.1 * s
        with np.errstate(all="ignore"):
            u2, v2 = fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy
        keep &= (u2 >= 0) & (u2 < w) & (v2 >= 0) & (v2 < h)
        X1 = np.concatenate([X1, X[keep]])
    X1 = X1[:n]
    X2 = s * (X1 @ R.T) + t
    px = np.stack([fx * X1[:, 0] / X1[:, 2] + cx, fy * X1[:, 1] / X1[:, 2] + cy,
                   fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], axis=1)
    px = px + rng.normal(0, noise_px, (n, 4)) if noise_px else px
    if depth_noise:
        X1 = X1 * (1.0 + depth_noise * rng.normal(0, 1, (n, 1)))
        X2 = X2 * (1.0 + depth_noise * rng.normal(0, 1, (n, 1)))
    truth = np.ones(n, bool)
    n_out = int(round(n * outliers))
    out_idx = rng.permutation(n)[:n_out]
    truth[out_idx] = False
    src = np.roll(out_idx, 1) if n_out > 1 else (out_idx + 1) % max(n, 1)
    X2o, pxo = X2.copy(), px.copy()
    X2[out_idx], px[out_idx, 2:] = X2o[src], pxo[src, 2:]
    corr = np.zeros(n, SIM3_CORR_DTYPE)
    corr["X1"], corr["X2"] = X1, X2
    corr["u1"], corr["v1"], corr["u2"], corr["v2"] = px[:, 0], px[:, 1], px[:, 2], px[:, 3]
    return corr, truth


rotation_error_deg = P.rotation_error_deg
rot = P.rot
