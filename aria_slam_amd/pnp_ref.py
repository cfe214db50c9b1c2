"""NumPy restatement of the absolute pose stage (include/aria_orb_hip.h, "absolute pose from the point map"; kernels in
aria_slam_amd/csrc/pnp_ransac.hip): the same sample hash, 6-point DLT, fp32 scoring, Gauss-Newton refinement and outputs.

The reference project has no PnP code, so this module is the definition the device is held to (tests/test_gpu_pnp.py over
the table of tests/pnp_cases.py); parity with OpenCV's solvePnPRansac is not claimed. The scoring runs in fp32 in the
device's order of operations; the solver and the refinement run in fp64 (3x3 SVD: LAPACK here, Jacobi on the device).

estimate(dtype=np.longdouble) is the yardstick that rounding is measured against (tools/pnp_gap.py): the refinement, the
nearest rotation it starts from and the outputs in extended precision; the hypotheses and every inlier test are the same
in both runs.

Two minimal solvers. solver="dlt" (the default) is the 6-point DLT above. solver="p3p" is a three-point solver with a fourth
point that picks among its roots (solve_p3p; MIN_CORR_P3P = 4 correspondences): the elimination of Persson and Nordberg
("Lambda Twist", ECCV 2018) restated with + - * / and sqrt alone -- one real root of the cubic by 30 Newton steps from a
start on the monotone side, the rank-2 form's eigenpairs from a quadratic and row cross products, up to four candidates in a
fixed order, five Newton steps on the distance equations each, the pose from the two triangles. No cbrt, acos or cos: their
results cannot be held between host and device. Parity with OpenCV's SOLVEPNP_P3P is not claimed. A plane through the
sample is no degeneracy of this solver, so a planar scene, where every DLT sample is invalid, yields a pose.

One model per hypothesis: the candidate that reprojects the sample's fourth point best. Scoring all roots would quadruple
the scoring loop; the price is that an outlier in slot 3 can pick the wrong root of an otherwise clean sample, and such a
hypothesis is lost. From the hand-over on -- scoring, winner, refinement (from 6 inliers), outputs -- the definition is the
one above; only the "fewer than 6 correspondences" gate becomes the solver's minimum."""
import numpy as np

from ._lib import KP_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE, PNP_CORR_DTYPE
from . import pose_ref as P
from .pose_ref import EUROC_K

PIVOT_TOL = 1e-9
RANK_TOL = 1e-9
RANGE = 1e15          # |X - X0|, |x|, |y| and |t0| beyond this never score: squares stay finite in fp32
MIN_CORR = 6
STEP_TOL = 1e-12
MIN_CORR_P3P = 4      # three points for the solver, the fourth picks among its roots
P3P_AREA_TOL = 1e-12  # |(X1 - X2) x (X1 - X3)|^2 <= tol * max(a_ij)^2: collinear or coincident sample points
P3P_CUBIC_STEPS = 30
P3P_POLISH_STEPS = 5
SOLVERS = ("dlt", "p3p")


def min_corr(solver="dlt"):
    if solver not in SOLVERS:
        raise ValueError("solver must be one of %r" % (SOLVERS,))
    return MIN_CORR if solver == "dlt" else MIN_CORR_P3P


def sample_indices(seed, pair, hypotheses, n, k=6):
    """(hypotheses, k) sample indices: the pose stage's hash with k slots (6 for the DLT, 4 for P3P)."""
    return P.sample_indices(seed, pair, hypotheses, n, k=k)


def threshold2(threshold_px=2.0, K=EUROC_K):
    t = threshold_px / ((K[0] + K[1]) * 0.5)
    return np.float32(t * t)


def as_corr(corr):
    c = np.ascontiguousarray(corr)
    if c.dtype != PNP_CORR_DTYPE:
        c = c.view(PNP_CORR_DTYPE)
    return c.reshape(-1)


def stage(corr, K=EUROC_K):
    """What k_pnp_stage leaves: xy (n, 2) fp64 normalised pixels, d32 (n, 3) and xy32 (n, 2) fp32 scoring values (all NaN for
    a correspondence with a value that is not finite or beyond RANGE), X (n, 3) fp64 and X0."""
    c = as_corr(corr)
    fx, fy, cx, cy = K
    n = len(c)
    X = c["X"].astype(np.float64).reshape(n, 3)
    xy = np.stack([(c["u"].astype(np.float64) - cx) / fx, (c["v"].astype(np.float64) - cy) / fy], axis=1).reshape(n, 2)
    X0 = X[0].copy() if n else np.zeros(3)
    with np.errstate(all="ignore"):
        d32 = (X - X0).astype(np.float32)
        xy32 = xy.astype(np.float32)
        bad = ~((np.abs(d32) <= np.float32(RANGE)).all(axis=1) & (np.abs(xy32) <= np.float32(RANGE)).all(axis=1))
    d32[bad] = np.nan
    xy32[bad] = np.nan
    return dict(X=X, xy=xy, d32=d32, xy32=xy32, X0=X0)


def rotation_from(M, dtype=None):
    """(R, sigma (3,) descending, ok) of one 3x3 M: R = U V^T of M = U S V^T; ok = sigma3 > RANK_TOL sigma1. dtype=None:
    LAPACK in fp64; otherwise the device's path in `dtype` -- V from the Jacobi eigenvectors of M^T M, u_i = M v_i / sigma_i,
    third columns as cross products."""
    if dtype is None:
        U, s, Vt = np.linalg.svd(np.asarray(M, np.float64))
        return U @ Vt, s, bool(s[2] > RANK_TOL * s[0])
    M = np.asarray(M, dtype)
    w, V = P.jacobi_eigh(M.T @ M, dtype)
    zero = dtype(0)
    s = np.array([np.sqrt(max(w[2], zero)), np.sqrt(max(w[1], zero)), np.sqrt(max(w[0], zero))], dtype)
    if not s[2] > dtype(RANK_TOL) * s[0]:
        return np.eye(3, dtype=dtype), s, False
    v1, v2 = V[:, 2], V[:, 1]
    u1, u2 = M @ v1 / s[0], M @ v2 / s[1]
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    return np.outer(u1, v1) + np.outer(u2, v2) + np.outer(u3, v3), s, True


def solve_minimal(X, xy):
    """6-point DLT on (H, 6, 3) world points and (H, 6, 2) normalised pixels, in the device's order of operations.
    Returns (R (H, 3, 3), t (H, 3), valid (H,)): x_cam = R X + t."""
    X = np.asarray(X, np.float64)
    xy = np.asarray(xy, np.float64)
    H = X.shape[0]
    ar = np.arange(H)
    with np.errstate(all="ignore"):
        c = np.zeros((H, 3))
        for i in range(6):
            c = c + X[:, i]
        c = c / 6.0
        s = np.zeros(H)
        for i in range(6):
            d = X[:, i] - c
            s = s + np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        s = s / 6.0
        ok = (s > 0) & np.isfinite(s)
        sd = np.where(ok, s, 1.0)
        A = np.zeros((H, 11, 12))
        for r in range(11):
            i, second = r // 2, r % 2
            Xh = np.concatenate([(X[:, i] - c) / sd[:, None], np.ones((H, 1))], axis=1)
            A[:, r, 4 * second:4 * second + 4] = Xh
            A[:, r, 8:12] = (-xy[:, i, second])[:, None] * Xh
        amax = np.abs(A).reshape(H, -1).max(axis=1)
        for col in range(11):
            a = np.abs(A[:, col:, col])
            a = np.where(np.isnan(a), -1.0, a)
            piv = col + np.argmax(a, axis=1)
            ok &= a.max(axis=1) > PIVOT_TOL * amax
            rc = A[:, col, :].copy()
            A[:, col, :] = A[ar, piv, :]
            A[ar, piv, :] = rc
            inv = 1.0 / np.where(ok, A[:, col, col], 1.0)
            f = A[:, col + 1:, col] * inv[:, None]
            A[:, col + 1:, col + 1:] = A[:, col + 1:, col + 1:] - f[:, :, None] * A[:, col, None, col + 1:]
        p = np.zeros((H, 12))
        p[:, 11] = 1.0
        for col in range(10, -1, -1):
            acc = np.zeros(H)
            for k in range(col + 1, 12):
                acc = acc + A[:, col, k] * p[:, k]
            p[:, col] = -acc / np.where(ok, A[:, col, col], 1.0)
        ok &= np.isfinite(p).all(axis=1)
        p[~ok] = 0.0
        Pm = p.reshape(H, 3, 4)
        M, m = Pm[:, :, :3], Pm[:, :, 3]
        det = (M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1])
               - M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0])
               + M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]))
        ok &= det > 0
        M = np.where(ok[:, None, None], M, np.eye(3)[None])
        U, sv, Vt = np.linalg.svd(M)
        ok &= sv[:, 2] > RANK_TOL * sv[:, 0]
        R = U @ Vt
        lam = (sv[:, 0] + sv[:, 1] + sv[:, 2]) / 3.0
        Rc = np.stack([(R[:, k, 0] * c[:, 0] + R[:, k, 1] * c[:, 1]) + R[:, k, 2] * c[:, 2] for k in range(3)], axis=1)
        t = sd[:, None] * (m / lam[:, None]) - Rc
        ok &= np.isfinite(R).all(axis=(1, 2)) & np.isfinite(t).all(axis=1)
    R[~ok] = 0.0
    t[~ok] = 0.0
    return R, t, ok


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _det3(c0, c1, c2):
    return _dot(c0, _cross(c1, c2))


def _rank2_vector(d, lam):
    """The null vector of D0 - lam I (d = the six entries d00 d01 d02 d11 d12 d22): the largest of the three row cross
    products (ties to the earliest), normalised."""
    r0 = (d[0] - lam, d[1], d[2])
    r1 = (d[1], d[3] - lam, d[4])
    r2 = (d[2], d[4], d[5] - lam)
    v, n = None, None
    for c in (_cross(r0, r1), _cross(r0, r2), _cross(r1, r2)):
        cn = _dot(c, c)
        if v is None:
            v, n = c, cn
        else:
            take = cn > n
            v = tuple(np.where(take, c[k], v[k]) for k in range(3))
            n = np.where(take, cn, n)
    nn = np.sqrt(n)
    return (v[0] / nn, v[1] / nn, v[2] / nn)


def solve_p3p(X, xy, dtype=np.float64, detail=False):
    """The P3P minimal solver on (H, 4, 3) world points and (H, 4, 2) normalised pixels, in `dtype` and in the device's
    order of operations: points 0..2 are solved, point 3 picks the candidate. Returns (R (H, 3, 3), t (H, 3), valid (H,),
    slot (H,)): x_cam = R X + t; slot = the chosen candidate, 2 * (sign of s: 0 = +s, 1 = -s) + (root of the tau quadratic:
    0 = q / A, 1 = C / q), -1 when invalid. detail=True appends a dict: `alive` (H, 4) the candidates that passed step 4,
    `usable` (H, 4) those that also passed step 7's tests, `lengths` (H, 4, 3) after the polish, `poses` (R (H, 4, 3, 3),
    t (H, 4, 3)), `a` (a12, a13, a23), `b` (b12, b13, b23), `bearings` (H, 3, 3), `err` (H, 4) the fourth point's error, `area2` and `amax`
    (the degeneracy test's two sides), `degenerate` (H,)."""
    dt = dtype
    X = np.asarray(X, dt)
    xy = np.asarray(xy, dt)
    H = X.shape[0]
    c = lambda v: dt(v)   # noqa: E731
    with np.errstate(all="ignore"):
        # 1. setup
        yb = []
        for i in range(3):
            x, y = xy[:, i, 0], xy[:, i, 1]
            nrm = np.sqrt((x * x + y * y) + c(1))
            yb.append((x / nrm, y / nrm, c(1) / nrm))
        Xs = [tuple(X[:, i, k] for k in range(3)) for i in range(4)]
        sub = lambda p, q: (p[0] - q[0], p[1] - q[1], p[2] - q[2])   # noqa: E731
        v1, v2, d23 = sub(Xs[0], Xs[1]), sub(Xs[0], Xs[2]), sub(Xs[1], Xs[2])
        a12, a13, a23 = _dot(v1, v1), _dot(v2, v2), _dot(d23, d23)
        b12, b13, b23 = _dot(yb[0], yb[1]), _dot(yb[0], yb[2]), _dot(yb[1], yb[2])
        # 6's degeneracy test, first: collinear or coincident sample points
        v3 = _cross(v1, v2)
        area2 = _dot(v3, v3)
        amax = np.maximum(np.maximum(a12, a13), a23)
        ok = area2 > c(P3P_AREA_TOL) * (amax * amax)
        # 2. the cubic det(D1 + g D2) = 0
        z = np.zeros(H, dt)
        D1 = ((a23, -(a23 * b12), z), (-(a23 * b12), a23 - a12, a12 * b23), (z, a12 * b23, -a12))       # columns (symmetric)
        D2 = ((a23, z, -(a23 * b13)), (z, -a13, a13 * b23), (-(a23 * b13), a13 * b23, a23 - a13))
        c3 = _det3(D2[0], D2[1], D2[2])
        c2 = (_det3(D1[0], D2[1], D2[2]) + _det3(D2[0], D1[1], D2[2])) + _det3(D2[0], D2[1], D1[2])
        c1 = (_det3(D2[0], D1[1], D1[2]) + _det3(D1[0], D2[1], D1[2])) + _det3(D1[0], D1[1], D2[2])
        c0 = _det3(D1[0], D1[1], D1[2])
        ok &= c3 != 0
        ca, cb, cc = c2 / c3, c1 / c3, c0 / c3
        xi = -ca / c(3)
        disc = ca * ca - c(3) * cb
        fi = ((xi + ca) * xi + cb) * xi + cc
        r = c(2) * np.sqrt(np.where(disc > 0, disc, c(0))) / c(3)
        g = np.where(disc > 0, np.where(fi > 0, xi - r, xi + r), xi)
        for _ in range(P3P_CUBIC_STEPS):
            f = ((g + ca) * g + cb) * g + cc
            fp = (c(3) * g + c(2) * ca) * g + cb
            g = np.where(fp != 0, g - f / np.where(fp != 0, fp, c(1)), g)
        # 3. the rank-2 form D0 = D1 + g D2
        d = (D1[0][0] + g * D2[0][0], D1[0][1] + g * D2[0][1], D1[0][2] + g * D2[0][2],
             D1[1][1] + g * D2[1][1], D1[1][2] + g * D2[1][2], D1[2][2] + g * D2[2][2])
        tr = (d[0] + d[3]) + d[5]
        mm = ((d[0] * d[3] - d[1] * d[1]) + (d[0] * d[5] - d[2] * d[2])) + (d[3] * d[5] - d[4] * d[4])
        dq = tr * tr - c(4) * mm
        sq = np.sqrt(np.where(dq > 0, dq, c(0)))
        la = (tr + np.where(tr >= 0, sq, -sq)) / c(2)
        lb = mm / la
        pos = la > 0
        ok &= (pos & (lb < 0)) | ((la < 0) & (lb > 0))
        ea, eb = _rank2_vector(d, la), _rank2_vector(d, lb)
        e1 = tuple(np.where(pos, ea[k], eb[k]) for k in range(3))
        e2 = tuple(np.where(pos, eb[k], ea[k]) for k in range(3))
        lpos, lneg = np.where(pos, la, lb), np.where(pos, lb, la)
        s = np.sqrt(np.where(ok, -lneg / lpos, c(0)))
        # 4. - 7. the four candidate slots, in order
        best_err = np.full(H, np.inf, dt)
        slot = np.full(H, -1, np.int64)
        Rb = [[np.zeros(H, dt) for _ in range(3)] for _ in range(3)]
        tb = [np.zeros(H, dt) for _ in range(3)]
        det = {k: [] for k in ("alive", "usable", "lengths", "R", "t", "err")}
        x4, y4 = xy[:, 3, 0], xy[:, 3, 1]
        for sign in range(2):
            ss = s if sign == 0 else -s
            p0, p1, p2 = e1[0] - ss * e2[0], e1[1] - ss * e2[1], e1[2] - ss * e2[2]
            w0, w1 = -p1 / p0, -p2 / p0
            A = a23 * (w1 * w1) - a12
            B = a23 * (c(2) * (w0 * w1) - c(2) * (b12 * w1)) + c(2) * (a12 * b23)
            C = a23 * ((w0 * w0 + c(1)) - c(2) * (b12 * w0)) - a12
            qd = B * B - c(4) * (A * C)
            sqd = np.sqrt(np.where(qd >= 0, qd, c(0)))
            q = -(B + np.where(B >= 0, sqd, -sqd)) / c(2)
            for root in range(2):
                tau = q / A if root == 0 else C / q
                den = (c(1) + tau * tau) - (c(2) * b23) * tau
                l2 = np.sqrt(a23 / np.where(den > 0, den, c(1)))
                l3 = tau * l2
                l1 = w0 * l2 + w1 * l3
                alive = ok & (qd >= 0) & (tau > 0) & (den > 0) & (l1 > 0)
                # 5. polish
                for _ in range(P3P_POLISH_STEPS):
                    r1 = ((l1 * l1 + l2 * l2) - (c(2) * b12) * (l1 * l2)) - a12
                    r2 = ((l1 * l1 + l3 * l3) - (c(2) * b13) * (l1 * l3)) - a13
                    r3 = ((l2 * l2 + l3 * l3) - (c(2) * b23) * (l2 * l3)) - a23
                    j00, j01 = c(2) * (l1 - b12 * l2), c(2) * (l2 - b12 * l1)
                    j10, j12 = c(2) * (l1 - b13 * l3), c(2) * (l3 - b13 * l1)
                    j21, j22 = c(2) * (l2 - b23 * l3), c(2) * (l3 - b23 * l2)
                    dj = -(j00 * (j12 * j21)) - j01 * (j10 * j22)
                    go = dj != 0
                    dd = np.where(go, dj, c(1))
                    # adj(J) r, J = [[j00 j01 0] [j10 0 j12] [0 j21 j22]]
                    e1_ = (-(j12 * j21) * r1 - (j01 * j22) * r2) + (j01 * j12) * r3
                    e2_ = (-(j10 * j22) * r1 + (j00 * j22) * r2) - (j00 * j12) * r3
                    e3_ = ((j10 * j21) * r1 - (j00 * j21) * r2) - (j01 * j10) * r3
                    l1 = np.where(go, l1 - e1_ / dd, l1)
                    l2 = np.where(go, l2 - e2_ / dd, l2)
                    l3 = np.where(go, l3 - e3_ / dd, l3)
                # 6. pose
                Y = [tuple(l * yb[i][k] for k in range(3)) for i, l in enumerate((l1, l2, l3))]
                u1, u2 = sub(Y[0], Y[1]), sub(Y[0], Y[2])
                u3 = _cross(u1, u2)
                iw = c(1) / np.where(ok, area2, c(1))
                wa, wb = _cross(v2, v3), _cross(v3, v1)
                w = [tuple(wa[k] * iw for k in range(3)), tuple(wb[k] * iw for k in range(3)), tuple(v3[k] * iw for k in range(3))]
                R = [[(u1[r_] * w[0][k] + u2[r_] * w[1][k]) + u3[r_] * w[2][k] for k in range(3)] for r_ in range(3)]
                t = [Y[0][r_] - ((R[r_][0] * Xs[0][0] + R[r_][1] * Xs[0][1]) + R[r_][2] * Xs[0][2]) for r_ in range(3)]
                # 7. choice by the fourth point
                Xc = [((R[r_][0] * Xs[3][0] + R[r_][1] * Xs[3][1]) + R[r_][2] * Xs[3][2]) + t[r_] for r_ in range(3)]
                zz = np.where(Xc[2] > 0, Xc[2], c(1))
                ex, ey = Xc[0] / zz - x4, Xc[1] / zz - y4
                err = ex * ex + ey * ey
                fin = np.isfinite(err)
                for r_ in range(3):
                    fin &= np.isfinite(t[r_])
                    for k in range(3):
                        fin &= np.isfinite(R[r_][k])
                usable = alive & fin & (Xc[2] > 0)
                take = usable & (err < best_err)
                best_err = np.where(take, err, best_err)
                slot = np.where(take, 2 * sign + root, slot)
                for r_ in range(3):
                    tb[r_] = np.where(take, t[r_], tb[r_])
                    for k in range(3):
                        Rb[r_][k] = np.where(take, R[r_][k], Rb[r_][k])
                if detail:
                    det["alive"].append(alive)
                    det["usable"].append(usable)
                    det["lengths"].append(np.stack([l1, l2, l3], axis=1))
                    det["R"].append(np.stack([np.stack(row, axis=1) for row in R], axis=1))
                    det["t"].append(np.stack(t, axis=1))
                    det["err"].append(err)
        valid = slot >= 0
        Rout = np.stack([np.stack(row, axis=1) for row in Rb], axis=1)
        tout = np.stack(tb, axis=1)
    Rout[~valid] = 0
    tout[~valid] = 0
    if not detail:
        return Rout, tout, valid, slot
    info = dict(alive=np.stack(det["alive"], axis=1), usable=np.stack(det["usable"], axis=1),
                lengths=np.stack(det["lengths"], axis=1), poses=(np.stack(det["R"], axis=1), np.stack(det["t"], axis=1)),
                err=np.stack(det["err"], axis=1), a=(a12, a13, a23), b=(b12, b13, b23),
                bearings=np.stack([np.stack(v, axis=1) for v in yb], axis=1), area2=area2, amax=amax,
                degenerate=~(area2 > c(P3P_AREA_TOL) * (amax * amax)))
    return Rout, tout, valid, slot, info


def scored_pose(R, t, X0):
    """(R32 (H, 9), t032 (H, 3), ok): the pose as scored, t0 = R X0 + t, rounded to fp32; ok = finite and |t0| <= RANGE."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t0 = np.stack([(R[:, k, 0] * X0[0] + R[:, k, 1] * X0[1]) + R[:, k, 2] * X0[2] + t[:, k] for k in range(3)], axis=1)
        ok = np.isfinite(R).all(axis=(1, 2)) & (np.abs(t0) <= RANGE).all(axis=1)
        R32 = R.reshape(-1, 9).astype(np.float32)
        t032 = np.where(ok[:, None], t0, 0.0).astype(np.float32)
    R32[~ok] = 0
    return R32, t032, ok


def _camera32(R32, t032, d32):
    R = np.asarray(R32, np.float32).reshape(-1, 9)
    t = np.asarray(t032, np.float32).reshape(-1, 3)
    d = np.asarray(d32, np.float32)
    dx, dy, dz = d[None, :, 0], d[None, :, 1], d[None, :, 2]
    with np.errstate(all="ignore"):
        return [((R[:, 3 * k, None] * dx + R[:, 3 * k + 1, None] * dy) + R[:, 3 * k + 2, None] * dz) + t[:, k, None]
                for k in range(3)]


def inliers32(R32, t032, d32, xy32, thr2):
    """(H, n) bool, the device's test in fp32 and its order: Xc = R d + t0; Xc.z > 0 and
    (Xc.x - x Xc.z)^2 + (Xc.y - y Xc.z)^2 <= thr2 Xc.z^2."""
    X, Y, Z = _camera32(R32, t032, d32)
    xy = np.asarray(xy32, np.float32)
    with np.errstate(all="ignore"):
        ex = X - xy[None, :, 0] * Z
        ey = Y - xy[None, :, 1] * Z
        return (Z > 0) & (ex * ex + ey * ey <= np.float32(thr2) * (Z * Z))


def error_ratio(R32, t032, d32, xy32, thr2):
    """(H, n) fp64: the squared error over thr2 z^2 (inf where z <= 0 or not finite) -- 1 at the threshold; the tests' band."""
    X, Y, Z = (a.astype(np.float64) for a in _camera32(R32, t032, d32))
    xy = np.asarray(xy32, np.float64)
    with np.errstate(all="ignore"):
        ex = X - xy[None, :, 0] * Z
        ey = Y - xy[None, :, 1] * Z
        r = (ex * ex + ey * ey) / (float(thr2) * Z * Z)
    return np.where((Z > 0) & np.isfinite(r), r, np.inf)


def hypotheses(corr, seed=0, pair=0, n_hyp=1024, threshold_px=2.0, K=EUROC_K, staged=None, solver="dlt", branches=None):
    """What aria_pnp_debug_hypotheses returns: (sample_idx (H, 6), R (H, 9) fp32, t0 (H, 3) fp32, counts (H,), -1 = invalid).
    solver="p3p": slots 4 and 5 of sample_idx are -1; `branches`, a list, receives the (H,) chosen candidate slots of
    solve_p3p (-1 where the hypothesis is invalid)."""
    st = staged if staged is not None else stage(corr, K)
    n = len(st["X"])
    k = min_corr(solver)
    idx = sample_indices(seed, pair, n_hyp, n, k=k)
    valid = (idx >= 0).all(axis=1)
    slots = np.full(n_hyp, -1, np.int64)
    R32 = np.zeros((n_hyp, 9), np.float32)
    t032 = np.zeros((n_hyp, 3), np.float32)
    counts = np.full(n_hyp, -1, np.int64)
    if valid.any():
        rows = np.flatnonzero(valid)
        if solver == "dlt":
            R, t, ok = solve_minimal(st["X"][idx[rows]], st["xy"][idx[rows]])
        else:
            R, t, ok, sl = solve_p3p(st["X"][idx[rows]], st["xy"][idx[rows]])
            slots[rows] = sl
        r32, t32, ok2 = scored_pose(R, t, st["X0"])
        ok &= ok2
        R32[rows[ok]] = r32[ok]
        t032[rows[ok]] = t32[ok]
        valid[rows[~ok]] = False
    if valid.any():
        thr2 = threshold2(threshold_px, K)
        live = np.flatnonzero(valid)
        for a in range(0, len(live), 256):
            sel = live[a:a + 256]
            counts[sel] = inliers32(R32[sel], t032[sel], st["d32"], st["xy32"], thr2).sum(axis=1)
    if k < 6:
        idx = np.concatenate([idx, np.full((n_hyp, 6 - k), -1, np.int64)], axis=1)
        slots[~valid] = -1
    if branches is not None:
        branches.append(slots)
    return idx, R32, t032, counts


def exp_so3(w, dtype=np.float64):
    """Rodrigues: I + a K + b K^2, a = sin(th) / th, b = (1 - cos(th)) / th^2 (series below th^2 = 1e-16)."""
    w = np.asarray(w, dtype)
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < dtype(1e-16):
        a, b = dtype(1) - th2 / dtype(6), dtype(0.5) - th2 / dtype(24)
    else:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (dtype(1) - np.cos(th)) / th2
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype)
    return np.eye(3, dtype=dtype) + a * Kx + b * (Kx @ Kx)


def residuals(R, t0, d, xy):
    """(n, 2) normalised reprojection residuals of Xc = R d + t0, in the arrays' dtype."""
    Xc = d @ R.T + t0
    return np.stack([Xc[:, 0] / Xc[:, 2] - xy[:, 0], Xc[:, 1] / Xc[:, 2] - xy[:, 1]], axis=1)


def gn_jacobian(R, t0, d):
    """(n, 2, 6): d residual / d (w, v) of the left update R <- Exp(w) R, t0 <- Exp(w) t0 + v, at (w, v) = 0."""
    Xc = d @ R.T + t0
    iz = 1 / Xc[:, 2]
    px, py = Xc[:, 0] * iz, Xc[:, 1] * iz
    J = np.zeros((len(d), 2, 6), Xc.dtype)
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2] = -(px * py), 1 + px * px, -py
    J[:, 0, 3], J[:, 0, 5] = iz, -(px * iz)
    J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = -(1 + py * py), px * py, px
    J[:, 1, 4], J[:, 1, 5] = iz, -(py * iz)
    return J


def cholesky_solve(A, b):
    """x of A x = b by Cholesky, in the arrays' dtype; None when a pivot is not positive or the solution is not finite."""
    n = len(b)
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
            if not d > 0 or not np.isfinite(d):
                return None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
        y = np.zeros_like(b)
        for i in range(n):
            y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
        x = np.zeros_like(b)
        for i in range(n - 1, -1, -1):
            x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x if np.isfinite(x.astype(np.float64)).all() else None


def refine(R, t0, d, xy, iters, dtype=np.float64):
    """Up to `iters` Gauss-Newton steps over a fixed point set. Returns (R, t0, steps taken)."""
    R, t0 = np.asarray(R, dtype), np.asarray(t0, dtype)
    done = 0
    for _ in range(iters):
        with np.errstate(all="ignore"):
            J = gn_jacobian(R, t0, d).reshape(-1, 6)
            r = residuals(R, t0, d, xy).reshape(-1)
            A, b = J.T @ J, J.T @ r
        if not (np.isfinite(A.astype(np.float64)).all() and np.isfinite(b.astype(np.float64)).all()):
            break
        delta = cholesky_solve(A, -b)
        if delta is None:
            break
        E = exp_so3(delta[:3], dtype)
        R, t0 = E @ R, E @ t0 + delta[3:]
        done += 1
        if np.sqrt((delta * delta).sum()) <= dtype(STEP_TOL):
            break
    return R, t0, done


def _invalid(n):
    return dict(R=np.eye(3), t=np.zeros(3), rms_px=0.0, n_corr=n, n_inliers=0, best_hypothesis=-1, iterations=0, refined=0,
                valid=0, mask=np.zeros(n, np.uint8), winner_R=None, winner_t0=None, refit_R=None, refit_t0=None, n_winner=0,
                n_refit=0)


def estimate(corr, seed=0, pair=0, n_hyp=1024, threshold_px=2.0, refine_iters=5, K=EUROC_K, dtype=None, hyp=None, staged=None,
             solver="dlt"):
    """aria_pnp_estimate on the CPU: a dict of the aria_pnp_result fields and the mask, plus what the tests need to judge a
    case: winner_R / winner_t0 (the winning pose as scored, fp32), refit_R / refit_t0 (the refined pose as rescored, fp32,
    whether or not it was kept; None without a refinement) and n_winner / n_refit. dtype=np.longdouble: the refinement and
    the outputs in extended precision. solver: the minimal solver of the hypotheses, and the least count a pair needs."""
    st = staged if staged is not None else stage(corr, K)
    n = len(st["X"])
    res = _invalid(n)
    if n < min_corr(solver):
        return res
    _idx, R32, t032, counts = hyp if hyp is not None else hypotheses(corr, seed, pair, n_hyp, threshold_px, K, st, solver)
    best = int(np.argmax(counts))
    if counts[best] < 0:
        return res
    dt = np.float64 if dtype is None else dtype
    thr2 = threshold2(threshold_px, K)
    inl = inliers32(R32[best], t032[best], st["d32"], st["xy32"], thr2)[0]
    n_win = int(inl.sum())
    Rk, t0k = R32[best].astype(dt).reshape(3, 3), t032[best].astype(dt)
    d, xy, X0 = (st["X"].astype(dt) - st["X0"].astype(dt)), st["xy"].astype(dt), st["X0"].astype(dt)
    final_inl, refined, iterations = inl, 0, 0
    refit_R = refit_t0 = None
    n_refit = 0
    if n_win >= MIN_CORR and refine_iters > 0:
        Rs, _s, ok = rotation_from(Rk, dtype)
        if ok:
            Rr, t0r, iterations = refine(Rs, t0k, d[inl], xy[inl], refine_iters, dt)
            if iterations:
                with np.errstate(all="ignore"):
                    r32 = Rr.astype(np.float64).reshape(1, 9).astype(np.float32)
                    t32 = t0r.astype(np.float64).reshape(1, 3).astype(np.float32)
                    good = bool(np.isfinite(r32).all() and (np.abs(t32) <= np.float32(RANGE)).all())
                if good:
                    inl_r = inliers32(r32, t32, st["d32"], st["xy32"], thr2)[0]
                    refit_R, refit_t0, n_refit = r32[0], t32[0], int(inl_r.sum())
                    if n_refit >= n_win:
                        Rk, t0k, final_inl, refined = Rr, t0r, inl_r, 1
    with np.errstate(all="ignore"):
        t = np.array([t0k[k] - ((Rk[k, 0] * X0[0] + Rk[k, 1] * X0[1]) + Rk[k, 2] * X0[2]) for k in range(3)], dt)
        n_in = int(final_inl.sum())
        rms = dt(0)
        if n_in:
            r = residuals(Rk, t0k, d[final_inl], xy[final_inl])
            rms = np.sqrt((r * r).sum() / dt(n_in)) * dt((K[0] + K[1]) * 0.5)
    if not (np.isfinite(Rk.astype(np.float64)).all() and np.isfinite(t.astype(np.float64)).all() and np.isfinite(float(rms))):
        return res
    res.update(R=Rk, t=t, rms_px=rms, n_inliers=n_in, best_hypothesis=best, iterations=iterations, refined=refined, valid=1,
               mask=final_inl.astype(np.uint8), winner_R=R32[best], winner_t0=t032[best], refit_R=refit_R, refit_t0=refit_t0,
               n_winner=n_win, n_refit=n_refit)
    return res


def associate(points, anchor_pair, anchor_view, kp_query, matches):
    """aria_pnp_associate_batch_device for one pair on the CPU: (corr, corr_match). The map points with pair == anchor_pair
    are looked up by their idx1 (anchor_view = 1) or idx2 (2); match m yields a correspondence when such a point has that
    index equal to m.train_idx -- of several, the one at the lowest arena position -- with the pixel of
    kp_query[m.query_idx]; match order is kept."""
    pts = np.asarray(points).view(MAP_POINT_DTYPE).reshape(-1)
    kq = np.asarray(kp_query).view(KP_DTYPE).reshape(-1)
    m = np.asarray(matches).view(MATCH_DTYPE).reshape(-1)
    key = pts["idx1"] if anchor_view == 1 else pts["idx2"]
    first = {}
    for pos in np.flatnonzero(pts["pair"] == anchor_pair):
        first.setdefault(int(key[pos]), int(pos))
    corr, back = [], []
    for i, a in enumerate(m):
        pos = first.get(int(a["train_idx"]))
        if pos is None:
            continue
        c = np.zeros(1, PNP_CORR_DTYPE)
        c["X"] = pts["X"][pos]
        c["u"], c["v"] = kq["x"][a["query_idx"]], kq["y"][a["query_idx"]]
        corr.append(c)
        back.append(i)
    return (np.concatenate(corr) if corr else np.zeros(0, PNP_CORR_DTYPE)), np.asarray(back, np.int32)


def synth_pnp(seed, n, R, t, outlier_frac=0.0, noise_px=0.5, K=EUROC_K, width=752, height=480, depth=(2.0, 20.0),
              offset=(0.0, 0.0, 0.0), planar=False):
    """Synthetic 3D-2D correspondences of a scene at 2-20 units in front of a camera with x_cam = R X + t, the world frame
    moved by `offset` (so the true pose is (R, t - R offset)). planar: every point on one tilted plane. The first
    round(n * outlier_frac) of a random permutation get random pixels.

    Returns (corr (PNP_CORR_DTYPE), inlier_truth (bool), R_true, t_true)."""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    R, t, offset = np.asarray(R, np.float64), np.asarray(t, np.float64), np.asarray(offset, np.float64)
    u = rng.uniform(0, width, n)
    v = rng.uniform(0, height, n)
    z = rng.uniform(depth[0], depth[1], n)
    xn, yn = (u - cx) / fx, (v - cy) / fy
    if planar:
        z = 6.0 / (1.0 - 0.3 * xn - 0.2 * yn)
    Xc = np.stack([xn * z, yn * z, z], axis=1)
    Xw = (Xc - t) @ R + offset                       # R^T (Xc - t), moved
    px = np.stack([u, v], axis=1) + rng.normal(0, noise_px, (n, 2))
    n_out = int(round(n * outlier_frac))
    truth = np.ones(n, bool)
    out_idx = rng.permutation(n)[:n_out]
    truth[out_idx] = False
    px[out_idx] = np.stack([rng.uniform(0, width, n_out), rng.uniform(0, height, n_out)], axis=1)
    corr = np.zeros(n, PNP_CORR_DTYPE)
    corr["X"] = Xw
    corr["u"], corr["v"] = px[:, 0], px[:, 1]
    return corr, truth, R, t - R @ offset


rotation_error_deg = P.rotation_error_deg
rot = P.rot
