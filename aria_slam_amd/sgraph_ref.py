"""NumPy restatement of the Sim(3) pose-graph stage and of the map correction after a loop (include/aria_orb_hip.h, "Sim(3)
pose-graph optimisation"): the roles of ORB-SLAM's OptimizeEssentialGraph and CorrectLoop. The reference has no code for
either, so this file is the definition the device kernels (csrc/sim3_graph.hip) and the tests follow. It is graph_ref.py with
a seventh coordinate: the SE(3) pieces, the LM control, PCG with block-Jacobi, the direct solver, check_graph and the
bookkeeping are imported from there, not copied.

Definitions (fp64 throughout; + - * / and sqrt only, no exp, log or acos)
  vertex    S = (R, t, s), camera-to-world: x_w = s R x_c + t. 13 doubles: R row-major, t, s (aria_sgraph_vertex).
            A B = (sA sB, RA RB, sA RA tB + tA);  S^-1 = (1/s, R^T, -(R^T t) / s).
  edge      (from, to, info_scale, Z 4x4 [R t], s): Z measures S_from^-1 S_to; information info_scale * I7.
  error     E = Z^-1 S_i^-1 S_j;  e = (t_E, qv_E, (s_E - 1/s_E) / 2), qv_E the vector part of quat_from_rot(R_E), w >= 0.
            The scale term is sinh(log s_E): odd under inversion, slope 1 at s_E = 1.  chi2 = sum info_scale * e.e.
  update    S <- S * D(d), D = (R(dq), dt, f(d7)) through from_mqt(d[:6]); f(x) = x + sqrt(x^2 + 1) for x >= 0 and
            1 / (-x + sqrt(x^2 + 1)) for x < 0: the inverse of the scale error, always positive, no cancellation. The
            rotation is then replaced by that of its unit quaternion, as in graph_ref.oplus.
  Jacobians with M = S_i^-1 S_j = (Rm, tm, sm), E = (Re, te, se), (v, w) the quaternion of Re, c = (se + 1/se) / 2:
              Ji = [[-Rz^T / sz, (2 / sz) Rz^T [tm]x, -Rz^T tm / sz], [0, -(w I - [v]x) Rz^T, 0], [0, 0, -c]]
              Jj = [[se Re, 0, 0], [0, w I + [v]x, 0], [0, 0, c]]
            With every scale 1 the upper-left 6x6 are graph_ref.edge_jacobians'.
  fix_scale the scale row of the error and the seventh row and column of both Jacobians are zero: the seventh row and column
            of every block and of b are zero, d7 = 0 exactly (f(0) = 1), every s comes back bit for bit.
  LM / PCG  graph_ref's, on 7x7 blocks; lambda0 = 1e-5 max diag(H) over the free vertices.
  invalid   graph_ref's rules, and a vertex s or an edge s that is not finite or <= 0: valid = 0, stop_reason 2, nothing
            written.
  map       correct_points: X' = S_new S_old^-1 X for every arena point whose pair has an anchor vertex, in one fixed
            operation order (below) so that the device computes the same bits.
"""
import numpy as np

from . import graph_ref as G
from .graph_ref import (MAX_TRIALS, STOP_INVALID, STOP_ITERATIONS, STOP_TRIALS, PoseGraph, check_graph, from_mqt,  # noqa: F401
                        quat_from_rot, rot_from_quat, skew)


# ---- Sim(3) ----------------------------------------------------------------------------------------------------------------
def make_vertex(R, t, s=1.0):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), [float(s)]])


def vertex_from_pose(T, s=1.0):
    """4x4 (or 3x4) camera-to-world [R t] -> vertex."""
    T = np.asarray(T, np.float64)
    return make_vertex(T[:3, :3], T[:3, 3], s)


def vertices_from_poses(poses, scales=None):
    poses = np.asarray(poses, np.float64)
    poses = poses.reshape(-1, poses.shape[-2], 4) if poses.size else poses.reshape(0, 4, 4)
    s = np.ones(len(poses)) if scales is None else np.asarray(scales, np.float64)
    return np.array([vertex_from_pose(p, k) for p, k in zip(poses, s)]).reshape(-1, 13)


def pose_of(S):
    """Vertex -> 4x4 [R t; 0 1], s dropped."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = S[:9].reshape(3, 3), S[9:12]
    return T


def poses_of(vertices):
    return np.array([pose_of(S) for S in np.asarray(vertices, np.float64).reshape(-1, 13)]).reshape(-1, 4, 4)


def parts(S):
    return S[:9].reshape(3, 3), S[9:12], S[12]


def mul(A, B):
    RA, tA, sA = parts(A)
    RB, tB, sB = parts(B)
    return make_vertex(RA @ RB, sA * (RA @ tB) + tA, sA * sB)


def inv(S):
    R, t, s = parts(S)
    return make_vertex(R.T, -(R.T @ t) / s, 1.0 / s)


def scale_error(s):
    """(s - 1/s) / 2 = sinh(log s)."""
    return (s - 1.0 / s) / 2


def f(x):
    """The inverse of scale_error: exp(asinh(x)) without either."""
    x = float(x)
    r = np.sqrt(x * x + 1.0)
    return x + r if x >= 0 else 1.0 / (-x + r)


def oplus(S, d):
    R, t, s = parts(S)
    D = from_mqt(d[:6])
    Rn = R @ D[:3, :3]
    Rn = rot_from_quat(quat_from_rot(Rn))
    return make_vertex(Rn, t + s * (R @ D[:3, 3]), s * f(d[6]))


def _edge_terms(Si, Sj, Z, sz):
    Ri, ti, si = parts(Si)
    Rj, tj, sj = parts(Sj)
    Rz, tz = Z[:3, :3], Z[:3, 3]
    Rm, tm, sm = Ri.T @ Rj, (Ri.T @ (tj - ti)) / si, sj / si
    Re, te, se = Rz.T @ Rm, (Rz.T @ (tm - tz)) / sz, sm / sz
    return Rz, tm, Re, te, se


def edge_error(Si, Sj, Z, sz=1.0, fix_scale=False):
    _Rz, _tm, Re, te, se = _edge_terms(Si, Sj, Z, sz)
    return np.concatenate([te, quat_from_rot(Re)[:3], [0.0 if fix_scale else scale_error(se)]])


def edge_jacobians(Si, Sj, Z, sz=1.0, fix_scale=False):
    """(e, Ji, Jj): the error and its analytic derivatives with respect to the updates of S_i and S_j."""
    Rz, tm, Re, te, se = _edge_terms(Si, Sj, Z, sz)
    q = quat_from_rot(Re)
    v, w = q[:3], q[3]
    RzT = Rz.T
    Ji, Jj = np.zeros((7, 7)), np.zeros((7, 7))
    Ji[:3, :3] = -RzT / sz
    Ji[:3, 3:6] = (2 * RzT @ skew(tm)) / sz
    Ji[3:6, 3:6] = -(w * np.eye(3) - skew(v)) @ RzT
    Jj[:3, :3] = se * Re
    Jj[3:6, 3:6] = w * np.eye(3) + skew(v)
    e7 = 0.0
    if not fix_scale:
        c = (se + 1.0 / se) / 2
        Ji[:3, 6] = -(RzT @ tm) / sz
        Ji[6, 6], Jj[6, 6] = -c, c
        e7 = scale_error(se)
    return np.concatenate([te, v, [e7]]), Ji, Jj


def numeric_jacobians(Si, Sj, Z, sz=1.0, h=1e-6):
    Ji, Jj = np.zeros((7, 7)), np.zeros((7, 7))
    for k in range(7):
        d = np.zeros(7)
        d[k] = h
        Ji[:, k] = (edge_error(oplus(Si, d), Sj, Z, sz) - edge_error(oplus(Si, -d), Sj, Z, sz)) / (2 * h)
        Jj[:, k] = (edge_error(Si, oplus(Sj, d), Z, sz) - edge_error(Si, oplus(Sj, -d), Z, sz)) / (2 * h)
    return Ji, Jj


# ---- graph as arrays ---------------------------------------------------------------------------------------------------------
# an edge is (from, to, info_scale, Z 4x4, s); a graph is (vertices (V, 13), edges, fixed index)
def norm_edges(edges):
    return [(int(e[0]), int(e[1]), float(e[2]), np.asarray(e[3], np.float64).reshape(-1, 4)[:3], float(e[4]) if len(e) > 4 else 1.0)
            for e in edges]


def check_sgraph(vertices, edges, fixed):
    """graph_ref.check_graph, and every vertex scale and every edge scale finite and positive."""
    if not check_graph(len(vertices), [e[:4] for e in edges], fixed):
        return False
    ok = lambda s: bool(np.isfinite(s) and s > 0)      # noqa: E731
    return all(ok(S[12]) for S in vertices) and all(ok(e[4]) for e in edges)


def chi2_of(vertices, edges, fix_scale=False):
    total = 0.0
    for i, j, w, Z, sz in edges:
        e = edge_error(vertices[i], vertices[j], Z, sz, fix_scale)
        total += w * (e @ e)
    return float(total)


def linearize(vertices, edges, fix_scale=False):
    """chi2, b (V, 7), the diagonal blocks D (V, 7, 7) and one off-diagonal block W_e = w Ji^T Jj (E, 7, 7) per edge (the
    block at (from, to)). Nothing of the fixed vertex is removed here."""
    V, E = len(vertices), len(edges)
    b, D, W = np.zeros((V, 7)), np.zeros((V, 7, 7)), np.zeros((E, 7, 7))
    chi2 = 0.0
    for k, (i, j, w, Z, sz) in enumerate(edges):
        e, Ji, Jj = edge_jacobians(vertices[i], vertices[j], Z, sz, fix_scale)
        chi2 += w * (e @ e)
        D[i] += w * Ji.T @ Ji
        D[j] += w * Jj.T @ Jj
        W[k] = w * Ji.T @ Jj
        b[i] -= w * Ji.T @ e
        b[j] -= w * Jj.T @ e
    return float(chi2), b, D, W


def optimize(vertices, edges, fixed=0, iterations=10, solver="pcg", pcg_max_iters=1000, pcg_rel_tol=1e-8, fix_scale=False):
    """graph_ref's Levenberg-Marquardt over Sim(3) vertices. Returns (vertices (V, 13), result dict as graph_ref.optimize's)."""
    vertices = np.array(vertices, np.float64).reshape(-1, 13).copy()
    edges = norm_edges(edges)
    res = dict(chi2_initial=0.0, chi2_final=0.0, lambda_=0.0, iterations_done=0, trials=0, pcg_iterations=0, valid=1,
               stop_reason=STOP_ITERATIONS, chi2_history=[], trace=[])
    if not check_sgraph(vertices, edges, fixed):
        res.update(valid=0, stop_reason=STOP_INVALID)
        return vertices, res
    if len(vertices) == 0:
        return vertices, res
    return G.lm_control(vertices, lambda S: linearize(S, edges, fix_scale), oplus, edges, fixed, iterations, solver,
                        pcg_max_iters, pcg_rel_tol, res)


# ---- the map after a loop ------------------------------------------------------------------------------------------------------
def correct_points(points, pair_vertex, pair_base, old, new):
    """ORB-SLAM's CorrectLoop on an arena: every MAP_POINT_DTYPE record whose pair p has pair_base <= p < pair_base + len(table)
    and v = pair_vertex[p - pair_base] >= 0 moves by X' = S_new[v] S_old[v]^-1 X in this operation order:
        d = X - t_old;  c_k = ((Ro[0][k] d0 + Ro[1][k] d1) + Ro[2][k] d2) / s_old
        X'_k = s_new * ((Rn[k][0] c0 + Rn[k][1] c1) + Rn[k][2] c2) + t_new_k
    Every other field is untouched. A point outside the table, or with v = -1, is left alone. A v outside the vertices, a
    used vertex whose s (old or new) is not finite or <= 0, or an X that is not finite, leaves the point alone and is counted
    as refused. Returns (points, (moved, left alone, refused))."""
    out = np.array(points, copy=True)
    table = np.asarray(pair_vertex, np.int64).reshape(-1)
    old = np.asarray(old, np.float64).reshape(-1, 13)
    new = np.asarray(new, np.float64).reshape(-1, 13)
    moved = left = refused = 0
    if len(out) == 0:
        return out, (0, 0, 0)
    slot = out["pair"].astype(np.int64) - int(pair_base)
    hit = (slot >= 0) & (slot < len(table))
    v = np.where(hit, table[np.clip(slot, 0, max(len(table) - 1, 0))] if len(table) else -1, -1)
    hit &= v >= 0
    left = int((~hit).sum())
    inside = hit & (v < min(len(old), len(new)))
    vv = np.where(inside, v, 0)
    X = out["X"].astype(np.float64)
    if len(old) and len(new):
        So, Sn = old[vv], new[vv]
        with np.errstate(all="ignore"):
            good = inside & np.isfinite(So[:, 12]) & (So[:, 12] > 0) & np.isfinite(Sn[:, 12]) & (Sn[:, 12] > 0) & \
                np.isfinite(X).all(1)
            d = X - So[:, 9:12]
            Ro, Rn = So[:, :9].reshape(-1, 3, 3), Sn[:, :9].reshape(-1, 3, 3)
            c = np.stack([((Ro[:, 0, k] * d[:, 0] + Ro[:, 1, k] * d[:, 1]) + Ro[:, 2, k] * d[:, 2]) / So[:, 12] for k in range(3)], 1)
            Y = np.stack([Sn[:, 12] * ((Rn[:, k, 0] * c[:, 0] + Rn[:, k, 1] * c[:, 1]) + Rn[:, k, 2] * c[:, 2]) + Sn[:, 9 + k]
                          for k in range(3)], 1)
    else:
        good, Y = np.zeros(len(out), bool), X
    moved = int(good.sum())
    refused = int((hit & ~good).sum())
    out["X"][good] = Y[good]
    return out, (moved, left, refused)


# ---- the bookkeeping -----------------------------------------------------------------------------------------------------------
class Sim3Graph(PoseGraph):
    """graph_ref.PoseGraph with a scale per edge: vertices enter as camera-to-world poses with s = 1; a loop edge carries the
    s of the alignment at the same x10. The optimised scales are kept beside the poses."""

    def clear(self):
        super().clear()
        self.scales = []

    def set_initial_pose(self, frame_id, pose):
        super().set_initial_pose(frame_id, pose)
        if len(self.scales) < len(self.poses):
            self.scales.append(1.0)
        else:
            self.scales[self.index[frame_id]] = 1.0

    def _add_edge(self, a, b, rel, info_scale, s=1.0):
        if not super()._add_edge(a, b, rel, info_scale):
            return False
        self.edges[-1] = self.edges[-1] + (float(s),)
        return True

    def add_loop_edge(self, from_id, to_id, relative_pose, s=1.0, info_scale=1.0):
        return self._add_edge(from_id, to_id, relative_pose, info_scale * self.LOOP_WEIGHT, s)

    def get_optimized_scale(self, frame_id):
        return self.scales[self.index[frame_id]] if frame_id in self.index else 1.0

    def vertices(self):
        return vertices_from_poses(np.array(self.poses), self.scales) if self.poses else np.zeros((0, 13))

    def _store(self, vertices):
        self.poses = [p for p in poses_of(vertices)]
        self.scales = [float(S[12]) for S in vertices]


class Sim3GraphOptimizer(Sim3Graph):
    """Sim3Graph + optimize() through this file's LM."""

    def __init__(self, solver="pcg", pcg_max_iters=1000, pcg_rel_tol=1e-8, fix_scale=False):
        super().__init__()
        self.solver, self.pcg_max_iters, self.pcg_rel_tol, self.fix_scale = solver, pcg_max_iters, pcg_rel_tol, fix_scale
        self.last_result = None

    def optimize(self, iterations=10):
        if not self.poses:
            return
        out, self.last_result = optimize(self.vertices(), self.edges, 0, iterations, self.solver, self.pcg_max_iters,
                                         self.pcg_rel_tol, self.fix_scale)
        self._store(out)


# ---- synthetic graphs ------------------------------------------------------------------------------------------------------------
def random_sgraph(seed, n_vertices, n_extra_edges=0, noise=0.05, scale_range=(0.5, 2.0), scale_noise=0.05):
    """graph_ref.random_graph's topology with a random scale per vertex in scale_range; measurements are the true relative
    similarities times a small random similarity."""
    rng = np.random.default_rng(seed)
    lo, hi = scale_range
    V = np.array([vertex_from_pose(G.random_pose(rng, 2.0), rng.uniform(lo, hi)) for _ in range(n_vertices)]).reshape(-1, 13)
    pairs = [(k, k + 1) for k in range(n_vertices - 1)]
    while len(pairs) < n_vertices - 1 + n_extra_edges and n_vertices > 2:
        a, b = rng.integers(0, n_vertices, 2)
        if a != b:
            pairs.append((int(a), int(b)))
    edges = []
    for a, b in pairs:
        Zs = mul(mul(inv(V[a]), V[b]), vertex_from_pose(G.random_pose(rng, noise, noise), 1.0 + rng.uniform(-scale_noise, scale_noise)))
        edges.append((a, b, float(rng.uniform(0.5, 10.0)), pose_of(Zs)[:3], float(Zs[12])))
    return V, edges
