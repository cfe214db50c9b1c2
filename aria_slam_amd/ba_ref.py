"""NumPy restatement of the local bundle-adjustment stage (include/aria_orb_hip.h, "local bundle adjustment"): the joint
refinement of the poses and points of one sliding window under Levenberg-Marquardt with a Schur complement over the
points. The reference has no code for it (its notes name the step: README.md:1162, H10_POSE_GRAPH_AUDIT.md:501-540), so this
file is the definition the device kernel (csrc/ba_schur.hip) and the tests follow. Parity with g2o or Ceres is not claimed.

Definitions (fp64 throughout)
  window    poses (P, 12): rows of the world-to-camera [R t], P <= 16, with a fixed byte each; points (N, 3) with a fixed
            byte each; observations OBS_DTYPE {point, pose, u, v} sorted strictly ascending by (point, pose); K = (fx, fy,
            cx, cy).
  invalid   an index out of range, an order that is not strictly ascending, P > 16, or a pose, point or pixel that is not
            finite: valid = 0, stop_reason = 2, nothing is changed.
  residual  Xc = R X + t, r = (fx Xc.x / Xc.z + cx - u, fy Xc.y / Xc.z + cy - v), e = |r|.
  used      an observation with Xc.z <= min_depth at the initial state is dropped for the whole call. A trial state at which
            a used observation has Xc.z <= min_depth, or whose chi2 is not finite, has chi2_new = inf.
  robust    Huber: w = 1 and the cost e^2 for e <= delta, else w = delta / e and the cost 2 delta e - delta^2; delta = 0
            switches it off. chi2 = sum of the costs over the used observations.
  update    pose: R <- Exp(w) R, t <- Exp(w) t + v (pnp_ref.exp_so3), parameters ordered (w, v); point: X <- X + dX.
  Jacobians A = d r / d Xc = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]], Jc = A [-[Xc]x  I] (2x6), Jp = A R (2x3).
  free      a pose that is not fixed; a point that is not fixed and has at least two used observations.
  system    U_i = sum w Jc^T Jc, V_j = sum w Jp^T Jp, W_o = w Jc^T Jp, bc_i = -sum w Jc^T r, bp_j = -sum w Jp^T r.
  step      Vd_j = V_j + lambda I (3x3 Cholesky, a non-positive pivot rejects the trial); over the free poses
            S_ik = [i == k](U_i + lambda I) - sum_j W_ij Vd_j^-1 W_kj^T, g_i = bc_i - sum_j W_ij Vd_j^-1 bp_j, solved by dense
            Cholesky (a non-positive pivot rejects the trial); dX_j = Vd_j^-1 (bp_j - sum_i W_ij^T dc_i).
  LM        graph_ref.optimize's: lambda0 = 1e-5 * the largest diagonal entry of U over the free poses and of V over the
            free points; rho = (chi2 - chi2_new) / (dx.(lambda dx + b) + 1e-3) over the free parameters; accepted when
            rho > 0 and chi2_new is finite: lambda *= max(1/3, 1 - (2 rho - 1)^3), ni = 2; else the state is restored,
            lambda *= ni, ni *= 2; ten rejected trials end the call (stop_reason 1). The state restarts per call.
  result    chi2_initial, chi2_final, lambda, rms_px = sqrt(sum e^2 / n_obs_used) at the final state, unweighted.
The summation order is not part of the definition: `reverse` takes every sum the other way round, which is what the tests use
to tell a decision that hangs on rounding from one that does not."""
import numpy as np

from ._lib import BA_OBS_DTYPE as OBS_DTYPE
from .pnp_ref import exp_so3
from .pose_ref import EUROC_K

STOP_ITERATIONS, STOP_TRIALS, STOP_INVALID = 0, 1, 2
MAX_TRIALS = 10
MAX_POSES = 16
HUBER_DEFAULT = float(np.sqrt(5.991))
MIN_DEPTH_DEFAULT = 1e-6


def make_window(poses, pose_fixed, points, point_fixed, obs, K=EUROC_K):
    return dict(poses=np.array(poses, np.float64).reshape(-1, 12), pose_fixed=np.array(pose_fixed, np.uint8).reshape(-1),
                points=np.array(points, np.float64).reshape(-1, 3), point_fixed=np.array(point_fixed, np.uint8).reshape(-1),
                obs=np.array(obs, OBS_DTYPE).reshape(-1), K=tuple(float(k) for k in K))


def check_window(win):
    P, N, obs = len(win["poses"]), len(win["points"]), win["obs"]
    if P > MAX_POSES or len(win["pose_fixed"]) != P or len(win["point_fixed"]) != N:
        return False
    pt, ps = obs["point"].astype(np.int64), obs["pose"].astype(np.int64)
    if len(obs) and not (np.all((pt >= 0) & (pt < N)) and np.all((ps >= 0) & (ps < P))):
        return False
    key = pt * MAX_POSES + ps
    if len(obs) > 1 and not np.all(key[1:] > key[:-1]):
        return False
    return bool(np.isfinite(win["poses"]).all() and np.isfinite(win["points"]).all() and np.isfinite(obs["u"]).all()
                and np.isfinite(obs["v"]).all())


def camera_points(poses, points, obs):
    """(n, 3) Xc of every observation."""
    T = poses.reshape(-1, 3, 4)[obs["pose"]]
    X = points[obs["point"]]
    return np.einsum("nab,nb->na", T[:, :, :3], X) + T[:, :, 3]


def residuals(poses, points, obs, K):
    """(r (n, 2), Xc (n, 3))."""
    fx, fy, cx, cy = K
    Xc = camera_points(poses, points, obs)
    with np.errstate(all="ignore"):
        r = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx - obs["u"].astype(np.float64),
                      fy * Xc[:, 1] / Xc[:, 2] + cy - obs["v"].astype(np.float64)], axis=1)
    return r, Xc


def jacobians(poses, points, obs, K):
    """(Jc (n, 2, 6), Jp (n, 2, 3)) for the updates of this file, at zero."""
    fx, fy, _cx, _cy = K
    Xc = camera_points(poses, points, obs)
    R = poses.reshape(-1, 3, 4)[obs["pose"]][:, :, :3]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    n = len(obs)
    A = np.zeros((n, 2, 3))
    A[:, 0, 0], A[:, 0, 2] = fx / z, -fx * x / (z * z)
    A[:, 1, 1], A[:, 1, 2] = fy / z, -fy * y / (z * z)
    B = np.zeros((n, 3, 6))                      # d Xc / d (w, v) = [-[Xc]x  I]
    B[:, 0, 1], B[:, 0, 2], B[:, 1, 0], B[:, 1, 2], B[:, 2, 0], B[:, 2, 1] = z, -y, -z, x, y, -x
    B[:, 0, 3] = B[:, 1, 4] = B[:, 2, 5] = 1.0
    return A @ B, A @ R


def apply_update(poses, points, dc, dX):
    out = poses.copy()
    for i in range(len(poses)):
        if np.any(dc[i] != 0):
            T = poses[i].reshape(3, 4)
            E = exp_so3(dc[i, :3])
            out[i] = np.concatenate([E @ T[:, :3], (E @ T[:, 3] + dc[i, 3:])[:, None]], axis=1).reshape(12)
    return out, points + dX


def huber_terms(r, delta):
    """(weight (n,), cost (n,), e2 (n,))."""
    e2 = (r * r).sum(1)
    e = np.sqrt(e2)
    if not delta > 0:
        return np.ones(len(r)), e2, e2
    out = e > delta
    with np.errstate(all="ignore"):
        w = np.where(out, delta / e, 1.0)
    return w, np.where(out, 2 * delta * e - delta * delta, e2), e2


def _sum(x, reverse):
    return float(np.sum(x[::-1] if reverse else x))


def _acc(n, idx, vals, reverse):
    out = np.zeros((n,) + vals.shape[1:])
    if reverse:
        idx, vals = idx[::-1], vals[::-1]
    np.add.at(out, idx, vals)
    return out


def used_mask(win, min_depth=MIN_DEPTH_DEFAULT):
    return camera_points(win["poses"], win["points"], win["obs"])[:, 2] > min_depth


def free_sets(win, used):
    """(free pose indices, free point indices)."""
    cnt = np.bincount(win["obs"]["point"][used], minlength=len(win["points"]))
    return np.flatnonzero(win["pose_fixed"] == 0), np.flatnonzero((win["point_fixed"] == 0) & (cnt >= 2))


def cost(poses, points, obs, K, used, huber, min_depth, reverse=False):
    """(chi2, sum e^2, smallest Xc.z) over the used observations; chi2 = inf where the state is rejected."""
    o = obs[used]
    r, Xc = residuals(poses, points, o, K)
    min_z = float(Xc[:, 2].min()) if len(o) else np.inf
    if not min_z > min_depth:
        return np.inf, np.inf, min_z
    _w, c, e2 = huber_terms(r, huber)
    chi2 = _sum(c, reverse)
    return (chi2, _sum(e2, reverse), min_z) if np.isfinite(chi2) else (np.inf, np.inf, min_z)


def system(poses, points, obs, K, used, huber, reverse=False):
    """The normal equations at a state: dict(chi2, U (P, 6, 6), bc (P, 6), V (N, 3, 3), bp (N, 3), W (n_used, 6, 3), o (the
    used observations))."""
    o = obs[used]
    P, N = len(poses), len(points)
    r, _Xc = residuals(poses, points, o, K)
    w, c, _e2 = huber_terms(r, huber)
    Jc, Jp = jacobians(poses, points, o, K)
    wJc, wJp = Jc * w[:, None, None], Jp * w[:, None, None]
    return dict(chi2=_sum(c, reverse), o=o,
                U=_acc(P, o["pose"], np.einsum("nra,nrb->nab", wJc, Jc), reverse),
                V=_acc(N, o["point"], np.einsum("nra,nrb->nab", wJp, Jp), reverse),
                W=np.einsum("nra,nrb->nab", wJc, Jp),
                bc=-_acc(P, o["pose"], np.einsum("nra,nr->na", wJc, r), reverse),
                bp=-_acc(N, o["point"], np.einsum("nra,nr->na", wJp, r), reverse))


def _dense_w(sysm, P, N):
    Wd = np.zeros((P, N, 6, 3))
    Wd[sysm["o"]["pose"], sysm["o"]["point"]] = sysm["W"]
    return Wd


def _cholesky(A):
    with np.errstate(all="ignore"):
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None
    return L if np.all(np.isfinite(L)) else None


def _cholesky_solve(L, b):
    try:
        from scipy.linalg import solve_triangular
    except ImportError:
        return np.linalg.solve(L.T, np.linalg.solve(L, b))
    return solve_triangular(L, solve_triangular(L, b, lower=True), lower=True, trans="T")


def reduced_system(sysm, fposes, fpoints, lam, reverse=False):
    """(S (6F, 6F), g (6F,), Vinv (M, 3, 3), Wf (F, M, 6, 3)) or None when some Vd is not positive definite."""
    P, N = len(sysm["U"]), len(sysm["V"])
    fpts = fpoints[::-1] if reverse else fpoints
    F, M = len(fposes), len(fpts)
    Vd = sysm["V"][fpts] + lam * np.eye(3)
    if M and _cholesky(Vd) is None:
        return None
    Vinv = np.linalg.inv(Vd) if M else np.zeros((0, 3, 3))
    Wf = _dense_w(sysm, P, N)[fposes][:, fpts]
    S = np.zeros((6 * F, 6 * F))
    for a, i in enumerate(fposes):
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = sysm["U"][i] + lam * np.eye(6)
    g = sysm["bc"][fposes].reshape(-1).copy()
    if F and M:
        A = np.einsum("fmab,mbc->fmac", Wf, Vinv).transpose(0, 2, 1, 3).reshape(6 * F, 3 * M)
        S -= A @ Wf.transpose(0, 2, 1, 3).reshape(6 * F, 3 * M).T
        g -= A @ sysm["bp"][fpts].reshape(-1)
    return S, g, Vinv, Wf, fpts


def solve_schur(sysm, fposes, fpoints, lam, reverse=False):
    """(dc (P, 6), dX (N, 3)) of the damped system through the reduced camera system, or None when a pivot fails."""
    P, N = len(sysm["U"]), len(sysm["V"])
    red = reduced_system(sysm, fposes, fpoints, lam, reverse)
    if red is None:
        return None
    S, g, Vinv, Wf, fpts = red
    dc, dX = np.zeros((P, 6)), np.zeros((N, 3))
    if len(fposes):
        L = _cholesky(S)
        if L is None:
            return None
        dc[fposes] = _cholesky_solve(L, g).reshape(-1, 6)
    if len(fpts):
        rhs = sysm["bp"][fpts] - np.einsum("fmab,fa->mb", Wf, dc[fposes])
        dX[fpts] = np.einsum("mab,mb->ma", Vinv, rhs)
    return dc, dX


def solve_full(sysm, fposes, fpoints, lam, reverse=False):
    """The same step from the undivided damped system, solved densely: the yardstick."""
    P, N = len(sysm["U"]), len(sysm["V"])
    F, M = len(fposes), len(fpoints)
    n = 6 * F + 3 * M
    H = np.zeros((n, n))
    Wf = _dense_w(sysm, P, N)[fposes][:, fpoints]
    for a, i in enumerate(fposes):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = sysm["U"][i]
    for b, j in enumerate(fpoints):
        H[6 * F + 3 * b:6 * F + 3 * b + 3, 6 * F + 3 * b:6 * F + 3 * b + 3] = sysm["V"][j]
    if F and M:
        H[:6 * F, 6 * F:] = Wf.transpose(0, 2, 1, 3).reshape(6 * F, 3 * M)
        H[6 * F:, :6 * F] = H[:6 * F, 6 * F:].T
    H[np.arange(n), np.arange(n)] += lam
    rhs = np.concatenate([sysm["bc"][fposes].reshape(-1), sysm["bp"][fpoints].reshape(-1)])
    dc, dX = np.zeros((P, 6)), np.zeros((N, 3))
    if n:
        L = _cholesky(H)
        if L is None:
            return None
        x = _cholesky_solve(L, rhs)
        dc[fposes], dX[fpoints] = x[:6 * F].reshape(-1, 6), x[6 * F:].reshape(-1, 3)
    return dc, dX


def linearize(win, lam, huber_px=HUBER_DEFAULT, min_depth=MIN_DEPTH_DEFAULT, reverse=False):
    """What aria_ba_debug_linearize returns: dict(chi2, n_obs_used, used, S, g, V, bp, free_poses, free_points); S and g are
    None when some Vd fails."""
    used = used_mask(win, min_depth)
    fposes, fpoints = free_sets(win, used)
    sysm = system(win["poses"], win["points"], win["obs"], win["K"], used, huber_px, reverse)
    red = reduced_system(sysm, fposes, fpoints, lam, False)
    return dict(chi2=sysm["chi2"], n_obs_used=int(used.sum()), used=used.astype(np.uint8), V=sysm["V"], bp=sysm["bp"],
                U=sysm["U"], bc=sysm["bc"], S=None if red is None else red[0], g=None if red is None else red[1],
                free_poses=fposes, free_points=fpoints)


def optimize(win, iterations=10, solver="schur", huber_px=HUBER_DEFAULT, min_depth=MIN_DEPTH_DEFAULT, reverse=False):
    """Levenberg-Marquardt as defined in the header of this file. Returns (poses (P, 12), points (N, 3), result): the fields
    of aria_ba_result plus used (the mask), trace, one entry per trial: dict(iteration, trial, rho, accepted, solved,
    lambda_ (before the trial), chi2_new, min_z (the smallest depth of a used observation at the
    trial state)), and history, the state after every accepted iteration: dict(poses, points,
    lambda_, chi2, rms_px, trials) -- a call with k iterations ends in history[k - 1] when the call got that far."""
    poses, points, obs, K = win["poses"].copy(), win["points"].copy(), win["obs"], win["K"]
    res = dict(chi2_initial=0.0, chi2_final=0.0, lambda_=0.0, rms_px=0.0, n_obs_used=0, iterations_done=0, trials=0,
               stop_reason=STOP_ITERATIONS, valid=1, used=np.zeros(len(obs), np.uint8), trace=[], history=[])
    if not check_window(win):
        res.update(valid=0, stop_reason=STOP_INVALID)
        return poses, points, res
    used = used_mask(win, min_depth)
    n_used = int(used.sum())
    res.update(used=used.astype(np.uint8), n_obs_used=n_used)
    fposes, fpoints = free_sets(win, used)
    step = solve_schur if solver == "schur" else solve_full
    sysm = system(poses, points, obs, K, used, huber_px, reverse)
    chi2 = sysm["chi2"]
    res["chi2_initial"] = chi2
    diag = [sysm["U"][i, k, k] for i in fposes for k in range(6)] + [sysm["V"][j, k, k] for j in fpoints for k in range(3)]
    lam, ni = 1e-5 * max(diag, default=0.0), 2.0
    rms = lambda e2: float(np.sqrt(e2 / n_used)) if n_used else 0.0    # noqa: E731
    e2sum = cost(poses, points, obs, K, used, huber_px, min_depth, reverse)[1] if n_used else 0.0
    for it in range(iterations):
        accepted = False
        for trial in range(MAX_TRIALS):
            res["trials"] += 1
            sol = step(sysm, fposes, fpoints, lam, reverse)
            rho, chi2_new, e2_new, min_z = 0.0, np.inf, np.inf, np.inf
            if sol is not None:
                dc, dX = sol
                tposes, tpoints = apply_update(poses, points, dc, dX)
                dcf, dXf = dc[fposes].reshape(-1), dX[fpoints].reshape(-1)
                if reverse:
                    dcf, dXf = dcf[::-1], dXf[::-1]
                scale = _sum(dcf * (lam * dcf + (sysm["bc"][fposes].reshape(-1)[::-1] if reverse else
                                                 sysm["bc"][fposes].reshape(-1))), False) + \
                    _sum(dXf * (lam * dXf + (sysm["bp"][fpoints].reshape(-1)[::-1] if reverse else
                                             sysm["bp"][fpoints].reshape(-1))), False) + 1e-3
                with np.errstate(all="ignore"):
                    chi2_new, e2_new, min_z = cost(tposes, tpoints, obs, K, used, huber_px, min_depth, reverse)
                    rho = float((chi2 - chi2_new) / scale)
            ok = bool(sol is not None and rho > 0 and np.isfinite(chi2_new))
            res["trace"].append(dict(iteration=it, trial=trial, rho=rho, accepted=ok, solved=sol is not None,
                                     lambda_=float(lam), chi2_new=float(chi2_new), min_z=min_z))
            if ok:
                poses, points, chi2, e2sum = tposes, tpoints, chi2_new, e2_new
                sysm = system(poses, points, obs, K, used, huber_px, reverse)
                lam *= max(1.0 / 3.0, 1.0 - (2 * rho - 1) ** 3)
                ni = 2.0
                accepted = True
                break
            lam *= ni
            ni *= 2
        if not accepted:
            res["stop_reason"] = STOP_TRIALS
            break
        res["iterations_done"] += 1
        res["history"].append(dict(poses=poses.copy(), points=points.copy(), lambda_=float(lam), chi2=float(chi2),
                                   rms_px=rms(e2sum), trials=res["trials"]))
    res.update(chi2_final=float(chi2), lambda_=float(lam), rms_px=rms(e2sum))
    return poses, points, res


def result_at(res, poses, points, k):
    """(poses, points, result fields) of a call with k >= 1 iterations, read from a longer call's history: the LM state is a
    function of the accepted iterations so far, so a shorter call is a prefix of a longer one."""
    fields = ("chi2_initial", "chi2_final", "lambda_", "rms_px", "n_obs_used", "iterations_done", "trials", "stop_reason",
              "valid")
    if k > len(res["history"]):               # the longer call ended before k iterations: so does the shorter one
        return poses, points, {f: res[f] for f in fields}
    h = res["history"][k - 1]
    return h["poses"], h["points"], dict(chi2_initial=res["chi2_initial"], chi2_final=h["chi2"], lambda_=h["lambda_"],
                                         rms_px=h["rms_px"], n_obs_used=res["n_obs_used"], iterations_done=k,
                                         trials=h["trials"], stop_reason=STOP_ITERATIONS, valid=res["valid"])


# ---- synthetic scenes ----------------------------------------------------------------------------------------------------------
def random_window(seed, poses=8, points=100, visibility="all", pixel_noise=0.5, pose_noise=0.02, point_noise=0.05,
                  outlier_share=0.0, K=EUROC_K, n_fixed=2, depth=(4.0, 12.0), step=0.5):
    """A camera moving sideways past a cloud `depth` units ahead. visibility: "all", or (lo, hi) poses per point. The first
    n_fixed poses are fixed and start at the truth; the others start pose_noise (radians and units) off, the points
    point_noise off. Pixels carry Gaussian pixel_noise; a share outlier_share of the observations is moved 50 to 200 px.
    Returns (window, truth dict(poses, points))."""
    rng = np.random.default_rng(seed)
    P, N = poses, points
    tp = np.zeros((P, 3, 4))
    for i in range(P):
        R = exp_so3(rng.normal(size=3) * 0.03)
        c = np.array([step * i, 0.05 * rng.normal(), 0.05 * rng.normal()])
        tp[i, :, :3], tp[i, :, 3] = R, -R @ c
    X = np.stack([rng.uniform(-3, 3 + step * P, N), rng.uniform(-2, 2, N), rng.uniform(depth[0], depth[1], N)], axis=1)
    idx = []
    for j in range(N):
        if visibility == "all":
            seen = range(P)
        else:
            lo, hi = visibility
            seen = sorted(rng.choice(P, size=int(rng.integers(lo, min(hi, P) + 1)), replace=False).tolist())
        idx += [(j, i) for i in seen]
    idx = np.array(idx, np.int64).reshape(-1, 2)
    obs = np.zeros(len(idx), OBS_DTYPE)
    obs["point"], obs["pose"] = idx[:, 0], idx[:, 1]
    r, _Xc = residuals(tp.reshape(-1, 12), X, obs, K)           # with u = v = 0: the projection itself
    px = r + rng.normal(0, pixel_noise, r.shape) if pixel_noise > 0 else r.copy()
    n_out = int(round(len(obs) * outlier_share))
    if n_out:
        which = rng.permutation(len(obs))[:n_out]
        ang, mag = rng.uniform(0, 2 * np.pi, n_out), rng.uniform(50, 200, n_out)
        px[which] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    obs["u"], obs["v"] = px[:, 0], px[:, 1]
    p0 = tp.copy()
    for i in range(n_fixed, P):
        E = exp_so3(rng.normal(size=3) * pose_noise)
        p0[i, :, :3], p0[i, :, 3] = E @ tp[i, :, :3], E @ tp[i, :, 3] + rng.normal(size=3) * pose_noise
    X0 = X + rng.normal(size=X.shape) * point_noise
    fixed = np.zeros(P, np.uint8)
    fixed[:n_fixed] = 1
    win = make_window(p0.reshape(-1, 12), fixed, X0, np.zeros(N, np.uint8), obs, K)
    return win, dict(poses=tp.reshape(-1, 12), points=X)


def truth_errors(poses, points, truth, win):
    """(mean translation error of the free poses' camera centres, mean error of the free points)."""
    def centres(p):
        T = p.reshape(-1, 3, 4)
        return -np.einsum("nba,nb->na", T[:, :, :3], T[:, :, 3])
    fp, fx = win["pose_fixed"] == 0, win["point_fixed"] == 0
    ep = np.linalg.norm(centres(poses) - centres(truth["poses"]), axis=1)[fp]
    ex = np.linalg.norm(points - truth["points"], axis=1)[fx]
    return (float(ep.mean()) if len(ep) else 0.0), (float(ex.mean()) if len(ex) else 0.0)


# ---- track builder -------------------------------------------------------------------------------------------------------------
def window_from_chain(arena, pair_first, n_pairs, kp1, n1, kp2, n2, matches, n_matches, point_cap, obs_cap,
                      query_is_first=True):
    """A window's points and observations from what the batch chain leaves behind. arena: MAP_POINT_DTYPE records; kp1 / kp2
    (n_pairs, kp_stride) KP_DTYPE, matches (n_pairs, match_cap) MATCH_DTYPE (query = view 1 when query_is_first) of the pairs
    pair_first .. pair_first + n_pairs - 1, as aria_map_triangulate_batch_device takes them. Frame f is view 1 of pair
    pair_first + f; the last frame is view 2 of the last pair. Integers and copies only.
    Returns dict(points (n, 3), obs, point_src (n,), n_points, n_obs, error): on an index out of
    range error = 1, on an overflow of a capacity error = 2, and the counts are 0."""
    from ._lib import MAP_POINT_DTYPE
    pts = np.asarray(arena).view(MAP_POINT_DTYPE).reshape(-1)
    fail = dict(points=np.zeros((0, 3)), obs=np.zeros(0, OBS_DTYPE), point_src=np.zeros(0, np.int32), n_points=0, n_obs=0,
                error=1)
    if not (1 <= n_pairs <= MAX_POSES - 1):
        return fail
    stride = kp1.shape[1]
    side1, side2 = ("query_idx", "train_idx") if query_is_first else ("train_idx", "query_idx")
    first = []                                    # per pair: view-1 index -> lowest match index
    for q in range(n_pairs):
        if not (0 <= n_matches[q] <= matches.shape[1] and 0 <= n1[q] <= stride and 0 <= n2[q] <= stride):
            return fail
        tab = {}
        for m in range(int(n_matches[q])):
            a, b = int(matches[q, m][side1]), int(matches[q, m][side2])
            if not (0 <= a < n1[q] and 0 <= b < n2[q]):
                return fail
            tab.setdefault(a, m)
        first.append(tab)
    X, src, obs = [], [], []
    for pos in np.flatnonzero((pts["pair"] >= pair_first) & (pts["pair"] < pair_first + n_pairs)):
        f = int(pts["pair"][pos]) - pair_first
        i1, i2 = int(pts["idx1"][pos]), int(pts["idx2"][pos])
        if not (0 <= i1 < n1[f] and 0 <= i2 < n2[f]):
            return fail
        j = len(X)
        X.append(pts["X"][pos])
        src.append(pos)
        obs.append((j, f, kp1[f, i1]["x"], kp1[f, i1]["y"]))
        obs.append((j, f + 1, kp2[f, i2]["x"], kp2[f, i2]["y"]))
        cur = i2
        for q in range(f + 1, n_pairs):
            m = first[q].get(cur)
            if m is None:
                break
            cur = int(matches[q, m][side2])
            obs.append((j, q + 1, kp2[q, cur]["x"], kp2[q, cur]["y"]))
    if len(X) > point_cap or len(obs) > obs_cap:
        return dict(fail, error=2)
    return dict(points=np.array(X, np.float64).reshape(-1, 3), obs=np.array(obs, OBS_DTYPE).reshape(-1),
                point_src=np.array(src, np.int32), n_points=len(X), n_obs=len(obs), error=0)
