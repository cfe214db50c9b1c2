"""NumPy restatement of the pose-graph stage (include/aria_orb_hip.h, "SE(3) pose-graph optimisation"): what the reference's
PoseGraphOptimizer (include/legacy/LoopClosure.hpp:80-113, src/legacy/LoopClosure.cpp:197-312) asks of g2o -- VertexSE3 /
EdgeSE3 under Levenberg-Marquardt, first vertex fixed, information info_scale * I6. This file is the specification the
device kernel (csrc/graph_optimize.hip) and the tests follow.

Parity with a running g2o is NOT pinned by any test: g2o and Eigen are not available to this project. The update rule, the
error, the LM control and its constants are g2o's as recalled, and are this project's definition as written here.

Definitions (fp64 throughout)
  pose      4x4 [R t; 0 1].
  fromMQT   d = (tx, ty, tz, qx, qy, qz) -> [R(q) t], q = (qx, qy, qz, w), w = sqrt(1 - |qv|^2); for |qv|^2 > 1 the
            quaternion is (w = 0, -qv) normalised.
  toMQT     T -> (t, qx, qy, qz) of the unit quaternion of R with w >= 0 (quat_from_rot: Shepperd's four branches, the trace
            branch when trace > 0, else the largest diagonal entry, first wins on ties; then normalised).
  update    X <- X * fromMQT(d); the rotation is then replaced by R(quat_from_rot(R)) (one re-orthonormalisation rule).
  error     e = toMQT(Z^-1 * Xi^-1 * Xj), chi2 = sum_e info_scale_e * e.e.
  Jacobians analytic, with E = Z^-1 Xi^-1 Xj = [Re te], its quaternion (v, w), M = Xi^-1 Xj = [Rm tm], Z = [Rz tz]:
              Ji = [[-Rz^T, 2 Rz^T [tm]x], [0, -(w I - [v]x) Rz^T]]      Jj = [[Re, 0], [0, w I + [v]x]]
  system    H = sum J^T (s I) J, b = -sum J^T (s e); the fixed vertex's rows and columns removed.
  LM        lambda0 = 1e-5 * max diag(H) at the first iteration of a call, ni = 2. A trial solves (H + lambda I) dx = b,
            applies the update and evaluates chi2_new; rho = (chi2 - chi2_new) / (dx.(lambda dx + b) + 1e-3). Accepted when
            rho > 0 and chi2_new is finite: lambda *= max(1/3, 1 - (2 rho - 1)^3), ni = 2. Otherwise the poses are restored,
            lambda *= ni, ni *= 2; at most 10 trials; an iteration whose trials all fail ends the call (stop_reason 1).
  PCG       block-Jacobi (inverse of the damped diagonal 6x6 blocks; a block whose Cholesky fails preconditions with 0),
            x0 = 0, stop at |r| <= rel_tol |b| or max_iters or p.Ap <= 0; |b| = 0 returns dx = 0 after 0 iterations.
  self-edges (from == to) are invalid input.
"""
import numpy as np

STOP_ITERATIONS, STOP_TRIALS, STOP_INVALID = 0, 1, 2
MAX_TRIALS = 10


# ---- SE(3) -----------------------------------------------------------------------------------------------------------------
def quat_from_rot(R):
    """Unit quaternion (x, y, z, w), w >= 0."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] >= R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q, np.float64)
    q = q / np.sqrt(q @ q)
    return -q if q[3] < 0 else q


def rot_from_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def from_mqt(d):
    d = np.asarray(d, np.float64)
    n2 = d[3:] @ d[3:]
    if n2 > 1.0:
        q = np.array([-d[3], -d[4], -d[5], 0.0]) / np.sqrt(n2)
    else:
        q = np.array([d[3], d[4], d[5], np.sqrt(1.0 - n2)])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot_from_quat(q), d[:3]
    return T


def to_mqt(T):
    return np.concatenate([T[:3, 3], quat_from_rot(T[:3, :3])[:3]])


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def oplus(X, d):
    Y = X @ from_mqt(d)
    Y[:3, :3] = rot_from_quat(quat_from_rot(Y[:3, :3]))
    Y[3] = (0, 0, 0, 1)
    return Y


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def edge_error(Xi, Xj, Z):
    return to_mqt(inv(Z) @ (inv(Xi) @ Xj))


def edge_jacobians(Xi, Xj, Z):
    """(e, Ji, Jj): the error and its analytic derivatives with respect to the updates of Xi and Xj."""
    M = inv(Xi) @ Xj
    E = inv(Z) @ M
    q = quat_from_rot(E[:3, :3])
    v, w = q[:3], q[3]
    RzT = Z[:3, :3].T
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3] = -RzT
    Ji[:3, 3:] = 2 * RzT @ skew(M[:3, 3])
    Ji[3:, 3:] = -(w * np.eye(3) - skew(v)) @ RzT
    Jj[:3, :3] = E[:3, :3]
    Jj[3:, 3:] = w * np.eye(3) + skew(v)
    return np.concatenate([E[:3, 3], v]), Ji, Jj


def numeric_jacobians(Xi, Xj, Z, h=1e-6):
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Ji[:, k] = (edge_error(oplus(Xi, d), Xj, Z) - edge_error(oplus(Xi, -d), Xj, Z)) / (2 * h)
        Jj[:, k] = (edge_error(Xi, oplus(Xj, d), Z) - edge_error(Xi, oplus(Xj, -d), Z)) / (2 * h)
    return Ji, Jj


# ---- graph as arrays ---------------------------------------------------------------------------------------------------------
# an edge is (from, to, info_scale, Z 4x4); a graph is (poses (V, 4, 4), edges, fixed index)
def check_graph(n, edges, fixed):
    if n > 0 and not (0 <= fixed < n):
        return False
    for i, j, s, _Z in edges:
        if not (0 <= i < n and 0 <= j < n) or i == j or not (np.isfinite(s) and s >= 0):
            return False
    return True


def chi2_of(poses, edges):
    total = 0.0
    for i, j, s, Z in edges:
        e = edge_error(poses[i], poses[j], Z)
        total += s * (e @ e)
    return float(total)


def linearize(poses, edges):
    """chi2, b (V, 6), the diagonal blocks D (V, 6, 6) and one off-diagonal block W_e = s Ji^T Jj (E, 6, 6) per edge (the
    block at (from, to); its transpose sits at (to, from)). Nothing of the fixed vertex is removed here."""
    V, E = len(poses), len(edges)
    b, D, W = np.zeros((V, 6)), np.zeros((V, 6, 6)), np.zeros((E, 6, 6))
    chi2 = 0.0
    for k, (i, j, s, Z) in enumerate(edges):
        e, Ji, Jj = edge_jacobians(poses[i], poses[j], Z)
        chi2 += s * (e @ e)
        D[i] += s * Ji.T @ Ji
        D[j] += s * Jj.T @ Jj
        W[k] = s * Ji.T @ Jj
        b[i] -= s * Ji.T @ e
        b[j] -= s * Jj.T @ e
    return float(chi2), b, D, W


def _matvec(D, W, ei, ej, lam, p):
    y = np.einsum("vab,vb->va", D, p) + lam * p
    np.add.at(y, ei, np.einsum("eab,eb->ea", W, p[ej]))
    np.add.at(y, ej, np.einsum("eba,eb->ea", W, p[ei]))
    return y


def block_jacobi(D, lam):
    """Inverse of the damped diagonal blocks; zero where the Cholesky factorisation fails."""
    Minv = np.zeros_like(D)
    for v in range(len(D)):
        A = D[v] + lam * np.eye(D.shape[-1])
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        if not np.all(np.isfinite(L)):
            continue
        Li = np.linalg.inv(L)
        Minv[v] = Li.T @ Li
    return Minv


def pcg(D, W, edges, b, lam, fixed, max_iters=1000, rel_tol=1e-8, precond=block_jacobi):
    """Preconditioned conjugate gradients on (H + lam I) dx = b with the fixed vertex removed. Returns (dx (V, 6), iters).
    The block size is that of D (6 here, 7 in sgraph_ref)."""
    V = len(D)
    ei = np.array([e[0] for e in edges], np.int64)
    ej = np.array([e[1] for e in edges], np.int64)
    free = np.ones((V, 1))
    if V:
        free[fixed] = 0
    Minv = precond(D, lam)
    x = np.zeros_like(b)
    r = b * free
    bb = float((r * r).sum())
    if bb == 0.0:
        return x, 0
    z = np.einsum("vab,vb->va", Minv, r)
    p = z.copy()
    rz = float((r * z).sum())
    iters = 0
    for k in range(1, max_iters + 1):
        Ap = _matvec(D, W, ei, ej, lam, p) * free
        pAp = float((p * Ap).sum())
        if not pAp > 0:
            break
        alpha = rz / pAp
        x += alpha * p
        r -= alpha * Ap
        iters = k
        z = np.einsum("vab,vb->va", Minv, r)
        rr, rz_new = float((r * r).sum()), float((r * z).sum())
        if rr <= rel_tol * rel_tol * bb:
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, iters


def direct(D, W, edges, b, lam, fixed):
    """Sparse LU of the same damped system (the stand-in for g2o's LinearSolverEigen; a dense solve where SciPy is not
    installed). Returns (dx, 0)."""
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
    except ImportError:
        sp = spl = None
    V, nb = len(D), D.shape[-1]                   # nb: the block size, 6 here and 7 in sgraph_ref
    free = [v for v in range(V) if v != fixed]
    pos = {v: k for k, v in enumerate(free)}
    n = nb * len(free)
    x = np.zeros((V, nb))
    if n == 0 or not np.any(b[free]):
        return x, 0
    rows, cols, vals = [], [], []

    def put(a, c, B):
        r0, c0 = nb * pos[a], nb * pos[c]
        rr, cc = np.meshgrid(np.arange(nb) + r0, np.arange(nb) + c0, indexing="ij")
        rows.append(rr.ravel()), cols.append(cc.ravel()), vals.append(B.ravel())
    for v in free:
        put(v, v, D[v] + lam * np.eye(nb))
    for k, (i, j) in enumerate((e[0], e[1]) for e in edges):
        if i in pos and j in pos:
            put(i, j, W[k])
            put(j, i, W[k].T)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    with np.errstate(all="ignore"):
        try:
            if sp is None:
                H = np.zeros((n, n))
                np.add.at(H, (rows, cols), vals)
                sol = np.linalg.solve(H, b[free].ravel())
            else:
                sol = spl.splu(sp.csc_matrix((vals, (rows, cols)), shape=(n, n))).solve(b[free].ravel())
        except (RuntimeError, np.linalg.LinAlgError):          # singular: no damping and a floating component
            return x, 0
    if np.all(np.isfinite(sol)):
        x[free] = sol.reshape(-1, nb)
    return x, 0


def optimize(poses, edges, fixed=0, iterations=10, solver="pcg", pcg_max_iters=1000, pcg_rel_tol=1e-8):
    """Levenberg-Marquardt as defined in the header of this file. Returns (poses (V, 4, 4), result dict with the fields of
    aria_graph_result plus chi2_history, the chi2 after every accepted iteration, and trace, one entry per trial:
    dict(iteration, trial, rho, accepted, lambda_ (before the trial), chi2_new, solver_iterations))."""
    poses = np.array(poses, np.float64).reshape(-1, 4, 4).copy()
    edges = [(int(i), int(j), float(s), np.asarray(Z, np.float64).reshape(4, 4)) for i, j, s, Z in edges]
    res = dict(chi2_initial=0.0, chi2_final=0.0, lambda_=0.0, iterations_done=0, trials=0, pcg_iterations=0, valid=1,
               stop_reason=STOP_ITERATIONS, chi2_history=[], trace=[])
    if not check_graph(len(poses), edges, fixed):
        res.update(valid=0, stop_reason=STOP_INVALID)
        return poses, res
    if len(poses) == 0:
        return poses, res
    return lm_control(poses, lambda P: linearize(P, edges), oplus, edges, fixed, iterations, solver, pcg_max_iters, pcg_rel_tol, res)


def lm_control(poses, linearize_fn, oplus_fn, edges, fixed, iterations, solver, pcg_max_iters, pcg_rel_tol, res):
    """The LM control of the header of this file over any vertex type: linearize_fn(vertices) -> (chi2, b, D, W) with square
    blocks of any one size, oplus_fn(vertex, d) -> vertex. `poses` is an array of vertices, copied per trial; `edges` is read
    for the vertex indices e[0], e[1] only. optimize() above and sgraph_ref.optimize() are its two callers."""
    chi2, b, D, W = linearize_fn(poses)
    res["chi2_initial"] = chi2
    free = [v for v in range(len(poses)) if v != fixed]
    lam = 1e-5 * max([D[v, k, k] for v in free for k in range(D.shape[-1])], default=0.0)
    ni = 2.0
    for _it in range(iterations):
        accepted = False
        for _trial in range(MAX_TRIALS):
            res["trials"] += 1
            if solver == "pcg":
                dx, n = pcg(D, W, edges, b, lam, fixed, pcg_max_iters, pcg_rel_tol)
            else:
                dx, n = direct(D, W, edges, b, lam, fixed)
            res["pcg_iterations"] += n
            trial = poses.copy()
            for v in free:
                trial[v] = oplus_fn(poses[v], dx[v])
            scale = float((dx[free] * (lam * dx[free] + b[free])).sum()) + 1e-3
            lin = linearize_fn(trial)
            rho = (chi2 - lin[0]) / scale
            ok = bool(rho > 0 and np.isfinite(lin[0]))
            res["trace"].append(dict(iteration=_it, trial=_trial, rho=float(rho), accepted=ok, lambda_=float(lam),
                                     chi2_new=float(lin[0]), solver_iterations=int(n)))
            if ok:
                poses = trial
                chi2, b, D, W = lin
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
        res["chi2_history"].append(chi2)
    res["chi2_final"], res["lambda_"] = chi2, lam
    return poses, res


# ---- the reference class's surface -------------------------------------------------------------------------------------------
class PoseGraph:
    """The bookkeeping of the reference's PoseGraphOptimizer, shared by this restatement and the device adapter: ids map to
    dense indices in the order they were first added (the first one added is the fixed vertex, LoopClosure.cpp:246-249);
    setInitialPose on a known id overwrites the estimate; an edge naming an unknown vertex is dropped silently (:258-261)."""
    LOOP_WEIGHT = 10.0

    def __init__(self):
        self.clear()

    def clear(self):
        self.index, self.poses, self.edges = {}, [], []

    def set_initial_pose(self, frame_id, pose):
        pose = np.array(pose, np.float64).reshape(4, 4)
        if frame_id in self.index:
            self.poses[self.index[frame_id]] = pose
        else:
            self.index[frame_id] = len(self.poses)
            self.poses.append(pose)

    def _add_edge(self, a, b, rel, info_scale):
        if a not in self.index or b not in self.index or a == b:    # a self-edge is invalid input of the stage: dropped too
            return False
        self.edges.append((self.index[a], self.index[b], float(info_scale), np.array(rel, np.float64).reshape(4, 4)))
        return True

    def add_odometry_edge(self, from_id, to_id, relative_pose, info_scale=1.0):
        return self._add_edge(from_id, to_id, relative_pose, info_scale)

    def add_loop_edge(self, from_id, to_id, relative_pose, info_scale=1.0):
        return self._add_edge(from_id, to_id, relative_pose, info_scale * self.LOOP_WEIGHT)

    def get_optimized_pose(self, frame_id):
        return self.poses[self.index[frame_id]].copy() if frame_id in self.index else np.eye(4)

    def get_all_poses(self):
        return [self.poses[self.index[k]].copy() for k in sorted(self.index)]


class PoseGraphOptimizer(PoseGraph):
    """PoseGraph + optimize() through this file's LM."""

    def __init__(self, solver="pcg", pcg_max_iters=1000, pcg_rel_tol=1e-8):
        super().__init__()
        self.solver, self.pcg_max_iters, self.pcg_rel_tol = solver, pcg_max_iters, pcg_rel_tol
        self.last_result = None

    def optimize(self, iterations=10):
        if not self.poses:
            return
        out, self.last_result = optimize(np.array(self.poses), self.edges, 0, iterations, self.solver, self.pcg_max_iters,
                                         self.pcg_rel_tol)
        self.poses = [p for p in out]


# ---- synthetic scenes ----------------------------------------------------------------------------------------------------------
def rot_axis(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = 0.5 * angle
    return rot_from_quat(np.concatenate([np.sin(h) * a, [np.cos(h)]]))


def make_pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def random_pose(rng, t_scale=1.0, angle=np.pi):
    return make_pose(rot_axis(rng.normal(size=3), rng.uniform(-angle, angle)), rng.normal(size=3) * t_scale)


def random_graph(seed, n_vertices, n_extra_edges=0, noise=0.05):
    """A chain with a few extra edges between random poses; measurements are the true relative poses times a small random
    motion, so residuals are small but not zero."""
    rng = np.random.default_rng(seed)
    poses = np.array([random_pose(rng, 2.0) for _ in range(n_vertices)]).reshape(-1, 4, 4)
    pairs = [(k, k + 1) for k in range(n_vertices - 1)]
    while len(pairs) < n_vertices - 1 + n_extra_edges and n_vertices > 2:
        a, b = rng.integers(0, n_vertices, 2)
        if a != b:
            pairs.append((int(a), int(b)))
    edges = []
    for a, b in pairs:
        Z = inv(poses[a]) @ poses[b] @ random_pose(rng, noise, noise)
        edges.append((a, b, float(rng.uniform(0.5, 10.0)), Z))
    return poses, edges


def circle_scene(seed, n=300, laps=1.1, radius=5.0, ripple=0.2, rot_noise=0.001, trans_noise=0.005, yaw_bias=0.0008,
                 n_loops=1):
    """The loop-closing scene: n vertices on `laps` laps of a circle with a vertical ripple; odometry = true relative motion
    with noise and a yaw bias per step; the initial poses are the odometry chained from the true first pose; n_loops loop
    edges one lap apart carrying the true relative pose. Returns (truth (n, 4, 4), initial (n, 4, 4), odometry edges,
    loop edges) with info_scale 1 on the odometry and 10 on the loops."""
    rng = np.random.default_rng(seed)
    per_lap = int(round(n / laps))
    truth = []
    for k in range(n):
        a = 2 * np.pi * k / per_lap
        t = np.array([radius * np.cos(a), radius * np.sin(a), ripple * np.sin(3 * a)])
        truth.append(make_pose(rot_axis([0, 0, 1], a + np.pi / 2), t))
    truth = np.array(truth)
    odo, init = [], [truth[0].copy()]
    for k in range(n - 1):
        rel = inv(truth[k]) @ truth[k + 1]
        err = make_pose(rot_axis(rng.normal(size=3), rng.normal() * rot_noise) @ rot_axis([0, 0, 1], yaw_bias),
                        rng.normal(size=3) * trans_noise)
        Z = rel @ err
        odo.append((k, k + 1, 1.0, Z))
        init.append(init[-1] @ Z)
    loops = []
    span = n - per_lap
    for k in range(n_loops):
        a = int(round(k * (span - 1) / max(n_loops - 1, 1))) if n_loops > 1 else span - 1
        loops.append((a, a + per_lap, 10.0, inv(truth[a]) @ truth[a + per_lap]))
    return truth, np.array(init), odo, loops


def ate(poses, truth):
    """RMS translation error without alignment (the reference's computeATE aligns nothing)."""
    d = np.asarray(poses)[:, :3, 3] - np.asarray(truth)[:, :3, 3]
    return float(np.sqrt((d * d).sum(1).mean()))
