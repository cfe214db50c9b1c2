"""NumPy restatement of trajectory evaluation (include/aria_orb_hip.h, "trajectory evaluation"), and its definition.

  sample_ground_truth   EuRoCReader::getGroundTruth (src/legacy/EuRoCReader.cpp:311-346): lower bound, clamps, lerp, slerp
  ate, rpe              computeATE / computeRPE (src/euroc_eval.cpp:28-61): no alignment
  svd3                  one-sided Jacobi SVD of a 3x3 matrix, on the matrix itself
  umeyama               alignment of an estimate onto the truth: none, rigid, similarity
  evaluate              everything aria_eval_result holds, for one trajectory

Everything is written in plain arithmetic on scalars of one dtype, so it runs in np.float64 (what the kernels compute, sums
in index order instead of their fixed tree) and in np.longdouble (the yardstick of tests/test_gpu_eval.py); numpy.linalg is
not used because it has no extended precision. Eigen's slerp is written out and is ours by definition."""
import numpy as np

ALIGN_NONE, ALIGN_SE3, ALIGN_SIM3 = 0, 1, 2
ALIGN_NAMES = {"none": ALIGN_NONE, "se3": ALIGN_SE3, "sim3": ALIGN_SIM3}
SLERP_EPS = 2.0 ** -52          # NumTraits<double>::epsilon(), in every dtype: a definition, not a rounding level
DEGENERATE_RATIO = 1e-10        # sigma2 <= this * sigma1: collinear or coincident points


# ---- ground truth ---------------------------------------------------------------------------------------------------------
def slerp(qa, qb, alpha, dtype=np.float64):
    """Eigen's QuaternionBase::slerp(alpha, other) on (w, x, y, z); not renormalised."""
    T = dtype
    a, b, alpha = np.asarray(qa, T), np.asarray(qb, T), T(alpha)
    d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
    ad = abs(d)
    if ad >= T(1) - T(SLERP_EPS):
        w0, w1 = T(1) - alpha, alpha
    else:
        th = np.arccos(ad)
        sth = np.sin(th)
        w0, w1 = np.sin((T(1) - alpha) * th) / sth, np.sin(alpha * th) / sth
    if d < 0:
        w1 = -w1
    return w0 * a + w1 * b


def ground_truth_valid(gt):
    """gt (M, 17): at least one row, every field finite, timestamps not decreasing."""
    gt = np.asarray(gt)
    return bool(len(gt) >= 1 and np.isfinite(gt.astype(np.float64)).all() and (gt[1:, 0] >= gt[:-1, 0]).all())


def sample_ground_truth(gt, timestamps, dtype=np.float64):
    """gt (M, 17) rows [t, p, q (w, x, y, z), v, bg, ba]; returns ((n, 17) samples, (n,) valid). An invalid table zeroes every
    output, a non-finite query its own."""
    T = dtype
    gt = np.asarray(gt, T).reshape(-1, 17)
    ts = np.asarray(timestamps, T).reshape(-1)
    out, valid = np.zeros((len(ts), 17), T), np.zeros(len(ts), np.int32)
    if not ground_truth_valid(gt):
        return out, valid
    for i, t in enumerate(ts):
        if not np.isfinite(t):
            continue
        lo, hi = 0, len(gt)
        while lo < hi:                       # std::lower_bound: first row with timestamp >= t
            mid = lo + ((hi - lo) >> 1)
            if gt[mid, 0] < t:
                lo = mid + 1
            else:
                hi = mid
        valid[i] = 1
        if lo == len(gt):
            out[i] = gt[-1]
        elif lo == 0:
            out[i] = gt[0]
        else:
            a, b = gt[lo - 1], gt[lo]
            alpha = (t - a[0]) / (b[0] - a[0])
            out[i, 0] = t
            for s in (slice(1, 4), slice(8, 11), slice(11, 14), slice(14, 17)):
                out[i, s] = (T(1) - alpha) * a[s] + alpha * b[s]
            out[i, 4:8] = slerp(a[4:8], b[4:8], alpha, T)
    return out, valid


# ---- metrics ----------------------------------------------------------------------------------------------------------------
def _sqnorm(d):
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _used(n, mask):
    return np.ones(n, bool) if mask is None else np.asarray(mask).reshape(n) != 0


def ate(est, truth, mask=None, dtype=np.float64):
    """computeATE over the used poses; -1 when there is none."""
    T = dtype
    e, g = np.asarray(est, T).reshape(-1, 3), np.asarray(truth, T).reshape(-1, 3)
    u = _used(len(e), mask)
    s, n = T(0), 0
    for i in range(len(e)):
        if u[i]:
            s += _sqnorm(e[i] - g[i])
            n += 1
    return np.sqrt(s / T(n)) if n else T(-1)


def rpe(est, truth, delta=10, mask=None, dtype=np.float64, scale=None, R=None):
    """computeRPE over the i >= delta whose two ends are both used; -1 without such a pair. With scale and R: of the aligned
    estimate (the translation cancels)."""
    T = dtype
    e, g = np.asarray(est, T).reshape(-1, 3), np.asarray(truth, T).reshape(-1, 3)
    u = _used(len(e), mask)
    s, n = T(0), 0
    for i in range(delta, len(e)):
        if u[i] and u[i - delta]:
            de = e[i] - e[i - delta]
            if R is not None:
                de = scale * _rot(R, de)
            s += _sqnorm(de - (g[i] - g[i - delta]))
            n += 1
    return (np.sqrt(s / T(n)) if n else T(-1)), n


def _rot(R, x):
    return np.array([(R[r, 0] * x[0] + R[r, 1] * x[1]) + R[r, 2] * x[2] for r in range(3)], R.dtype)


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])) + \
        M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0])


def svd3(M, dtype=np.float64, max_sweeps=30):
    """One-sided (Hestenes) Jacobi on M itself: returns (A, sigma, V) with M V = A, the columns of A orthogonal, sigma their
    lengths sorted descending. U's columns are A's divided by sigma where sigma > 0."""
    T = dtype
    A, V = np.array(M, T).reshape(3, 3), np.eye(3, dtype=T)
    eps = T(np.finfo(T).eps)
    for _ in range(max_sweeps):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = _sqnorm(A[:, p]), _sqnorm(A[:, q]), \
                (A[0, p] * A[0, q] + A[1, p] * A[1, q]) + A[2, p] * A[2, q]
            if not abs(gamma) > eps * np.sqrt(alpha * beta):
                continue
            zeta = (beta - alpha) / (T(2) * gamma)
            t = (T(1) if zeta >= 0 else T(-1)) / (abs(zeta) + np.sqrt(T(1) + zeta * zeta))
            c = T(1) / np.sqrt(T(1) + t * t)
            s = c * t
            for Mx in (A, V):
                xp, xq = Mx[:, p].copy(), Mx[:, q].copy()
                Mx[:, p] = c * xp - s * xq
                Mx[:, q] = s * xp + c * xq
            rotated = True
        if not rotated:
            break
    sg = np.array([np.sqrt(_sqnorm(A[:, c])) for c in range(3)], T)
    for p, q in ((0, 1), (0, 2), (1, 2)):
        if sg[p] < sg[q]:
            sg[[p, q]] = sg[[q, p]]
            A[:, [p, q]] = A[:, [q, p]]
            V[:, [p, q]] = V[:, [q, p]]
    return A, sg, V


def umeyama(est, truth, mode=ALIGN_SIM3, mask=None, dtype=np.float64):
    """Alignment of est onto truth over the used poses. Returns dict(valid, scale, R, t, sigma, n, det_sign)."""
    T = dtype
    e, g = np.asarray(est, T).reshape(-1, 3), np.asarray(truth, T).reshape(-1, 3)
    idx = np.nonzero(_used(len(e), mask))[0]
    n = len(idx)
    out = dict(valid=False, scale=T(-1), R=np.full((3, 3), T(-1)), t=np.full(3, T(-1)), sigma=np.zeros(3, T), n=n, det_sign=T(1))
    if n == 0:
        return out
    se, sg_ = np.zeros(3, T), np.zeros(3, T)
    for i in idx:
        se += e[i]
        sg_ += g[i]
    mu_e, mu_g = se / T(n), sg_ / T(n)
    Cm, var = np.zeros((3, 3), T), T(0)
    for i in idx:
        x, y = e[i] - mu_e, g[i] - mu_g
        for r in range(3):
            for c in range(3):
                Cm[r, c] += y[r] * x[c]
        var += _sqnorm(x)
    Cm, var = Cm / T(n), var / T(n)
    A, sg, V = svd3(Cm, T)
    out["sigma"] = sg
    if mode == ALIGN_NONE:
        out.update(valid=True, scale=T(1), R=np.eye(3, dtype=T), t=np.zeros(3, T))
        return out
    if n < 3 or not sg[1] > T(DEGENERATE_RATIO) * sg[0]:
        return out
    U = np.zeros((3, 3), T)
    U[:, 0], U[:, 1] = A[:, 0] / sg[0], A[:, 1] / sg[1]
    U[0, 2] = U[1, 0] * U[2, 1] - U[2, 0] * U[1, 1]        # u1 x u2: det [u1 u2 u3] = +1 whatever A's third column is
    U[1, 2] = U[2, 0] * U[0, 1] - U[0, 0] * U[2, 1]
    U[2, 2] = U[0, 0] * U[1, 1] - U[1, 0] * U[0, 1]
    du = T(-1) if ((A[0, 2] * U[0, 2] + A[1, 2] * U[1, 2]) + A[2, 2] * U[2, 2]) < 0 else T(1)   # det U of the full SVD
    dv = T(-1) if _det3(V) < 0 else T(1)
    d = du * dv
    R = np.zeros((3, 3), T)
    for r in range(3):
        for c in range(3):
            R[r, c] = (U[r, 0] * V[c, 0] + U[r, 1] * V[c, 1]) + (U[r, 2] * dv) * V[c, 2]
    scale = ((sg[0] + sg[1]) + d * sg[2]) / var if mode == ALIGN_SIM3 else T(1)
    t = mu_g - scale * _rot(R, mu_e)
    out.update(valid=True, scale=scale, R=R, t=t, det_sign=d)
    return out


def evaluate(est, truth, mode=ALIGN_SIM3, delta=10, mask=None, dtype=np.float64):
    """One trajectory: the fields of aria_eval_result (R as 3x3) plus pose_err (per pose, -1 where not used / not aligned).
    Non-finite used positions or delta < 1: valid = 0 and everything zero."""
    T = dtype
    e, g = np.asarray(est, T).reshape(-1, 3), np.asarray(truth, T).reshape(-1, 3)
    n_poses = len(e)
    u = _used(n_poses, mask)
    if len(g) != n_poses or delta < 1 or mode not in (0, 1, 2) or \
            not (np.isfinite(e[u].astype(np.float64)).all() and np.isfinite(g[u].astype(np.float64)).all()):
        return dict(valid=0, ate_raw=T(0), rpe_raw=T(0), scale=T(0), R=np.zeros((3, 3), T), t=np.zeros(3, T), sigma=np.zeros(3, T),
                    ate_rmse=T(0), ate_mean=T(0), ate_max=T(0), rpe_aligned=T(0), n_poses=0, n_used=0, n_rpe_pairs=0,
                    align_valid=0, pose_err=np.zeros(n_poses, T))
    al = umeyama(e, g, mode, mask, T)
    rpe_raw, pairs = rpe(e, g, delta, mask, T)
    res = dict(valid=1, ate_raw=ate(e, g, mask, T), rpe_raw=rpe_raw, scale=al["scale"], R=al["R"], t=al["t"], sigma=al["sigma"],
               n_poses=n_poses, n_used=al["n"], n_rpe_pairs=pairs, align_valid=int(al["valid"]), pose_err=np.full(n_poses, T(-1)))
    if not al["valid"]:
        res.update(ate_rmse=T(-1), ate_mean=T(-1), ate_max=T(-1), rpe_aligned=T(-1))
        return res
    s2, s1, mx = T(0), T(0), T(0)
    for i in range(n_poses):
        if u[i]:
            d = (al["scale"] * _rot(al["R"], e[i]) + al["t"]) - g[i]
            q = _sqnorm(d)
            err = np.sqrt(q)
            res["pose_err"][i] = err
            s2 += q
            s1 += err
            mx = max(mx, err)
    n = T(al["n"])
    res.update(ate_rmse=np.sqrt(s2 / n), ate_mean=s1 / n, ate_max=mx,
               rpe_aligned=rpe(e, g, delta, mask, T, al["scale"], al["R"])[0])
    return res


# ---- tracks -----------------------------------------------------------------------------------------------------------------
def rotation_from_axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt(a @ a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def truth_track(kind, n, rng):
    """Named truth shapes (n, 3), metres: 'walk' (random walk), 'circle' (near-planar circle, two nearly equal singular
    values), 'corridor' (sigma2 / sigma1 of the covariance about 1e-5)."""
    if kind == "walk":
        return np.cumsum(rng.normal(size=(n, 3)) * 0.05, axis=0)
    if kind == "circle":
        th = np.linspace(0, 2 * np.pi, n, endpoint=False)
        return np.stack([3 * np.cos(th), 3 * np.sin(th), 0.01 * rng.normal(size=n)], axis=1)
    if kind == "corridor":
        x = np.linspace(0, 40, n)
        return np.stack([x, 0.04 * rng.normal(size=n), 0.04 * rng.normal(size=n)], axis=1) * [1, 1, 0.5]
    raise ValueError(kind)


def make_track(kind, n, seed, scale=0.37, noise=0.01):
    """(est, truth, (scale, R, t)): truth of the named shape; est = the known similarity transform taken backwards, so that
    truth = scale R est + t up to the noise (metres, added to est)."""
    rng = np.random.default_rng(seed)
    g = truth_track(kind, n, rng)
    R = rotation_from_axis_angle(rng.normal(size=3), rng.uniform(0.3, 2.5))
    t = rng.normal(size=3) * 2
    e = ((g - t) @ R) / scale + noise * rng.normal(size=(n, 3))       # R^T (g - t) / s
    return e, g, (scale, R, t)


def truth_rows(n, seed, t0=100.0, dt=0.005):
    """n ground-truth rows (n, 17) with increasing timestamps and unit quaternions along a smooth motion."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 17))
    rows[:, 0] = t0 + dt * np.arange(n) + rng.uniform(0, 0.2 * dt, n)
    rows[:, 1:4] = np.cumsum(rng.normal(size=(n, 3)) * 0.01, axis=0)
    q = np.cumsum(rng.normal(size=(n, 4)) * 0.02, axis=0) + [1, 0, 0, 0]
    rows[:, 4:8] = q / np.sqrt((q * q).sum(1))[:, None]
    rows[:, 8:17] = rng.normal(size=(n, 9)) * 0.1
    return rows


# ---- the named tracks of tests/test_gpu_eval.py and tools/eval_gap.py -------------------------------------------------------
TRACK_NAMES = ("walk", "circle", "long", "masked", "short", "corridor")
METRE_FIELDS = ("ate_raw", "rpe_raw", "ate_rmse", "ate_mean", "ate_max", "rpe_aligned")


def named_track(name):
    """(est (n, 3), truth (n, 3), mask or None, delta) of a named track."""
    if name == "walk":
        e, g, _ = make_track("walk", 2000, 11)
        return e, g, None, 10
    if name == "circle":
        e, g, _ = make_track("circle", 1500, 12)
        return e, g, None, 10
    if name == "long":
        e, g, _ = make_track("walk", 65536, 13)
        return e, g, None, 10
    if name == "masked":
        e, g, _ = make_track("walk", 1200, 14)
        rng = np.random.default_rng(15)
        mask = (rng.uniform(size=len(e)) > 0.3).astype(np.uint8)
        e[mask == 0] = 1e3 * rng.normal(size=(int((mask == 0).sum()), 3))      # what a masked pose holds must not matter
        return e, g, mask, 10
    if name == "short":
        e, g, _ = make_track("walk", 12, 16, noise=0.002)
        return e, g, None, 10
    if name == "corridor":
        e, g, _ = make_track("corridor", 3000, 17)
        return e, g, None, 10
    raise ValueError(name)


def result_gap(a, b, positions):
    """Largest differences between two evaluate() results, by the three kinds of field: (metres: the metric fields, t and
    the per-pose errors, absolute; R and scale, absolute; sigma, relative to b's). Floored at one unit in the last place of
    fp64 at the magnitude involved (2^-52 times the largest coordinate for the metre fields), so that an agreement closer
    than the format can express does not turn into a bound of zero."""
    f = lambda x: np.asarray(x, np.longdouble)
    m = max([abs(f(a[k]) - f(b[k])) for k in METRE_FIELDS] + [np.abs(f(a["t"]) - f(b["t"])).max(),
                                                               np.abs(f(a["pose_err"]) - f(b["pose_err"])).max()])
    r = max(np.abs(f(a["R"]) - f(b["R"])).max(), abs(f(a["scale"]) - f(b["scale"])))
    s = (np.abs(f(a["sigma"]) - f(b["sigma"])) / f(b["sigma"])).max()
    ulp = 2.0 ** -52
    return (max(float(m), ulp * float(np.abs(positions).max())), max(float(r), ulp), max(float(s), ulp))


def track_gap(name, mode=ALIGN_SIM3):
    """GAP of a named track: its fp64 run against its np.longdouble run. Returns ((metres, R / scale, sigma), extended run)."""
    e, g, mask, delta = named_track(name)
    lo = evaluate(e, g, mode, delta, mask, np.float64)
    hi = evaluate(e, g, mode, delta, mask, np.longdouble)
    return result_gap(lo, hi, np.concatenate([e if mask is None else e[mask != 0], g])), hi


def sampler_case():
    """(gt rows (M, 17), queries): 36 000 rows, queries before, inside (exact hits among them) and after the span."""
    gt = truth_rows(36000, 21)
    rng = np.random.default_rng(22)
    inside = rng.uniform(gt[0, 0], gt[-1, 0], 500)
    q = np.concatenate([[gt[0, 0] - 1.0, gt[0, 0]], inside, gt[[1, 777, 35999], 0], [gt[-1, 0] + 1e-3, gt[-1, 0] + 5.0]])
    return gt, q


def sampler_gap():
    """GAP of the sampler case: fp64 against np.longdouble, absolute over all 17 fields (floored at 2^-52 times the largest
    field sampled apart from the timestamp, which is copied). Returns (gap, extended samples)."""
    gt, q = sampler_case()
    lo, _ = sample_ground_truth(gt, q, np.float64)
    hi, _ = sample_ground_truth(gt, q, np.longdouble)
    d = float(np.abs(lo[:, 1:].astype(np.longdouble) - hi[:, 1:]).max())
    return max(d, 2.0 ** -52 * float(np.abs(gt[:, 1:]).max())), hi
