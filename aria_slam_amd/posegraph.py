"""SE(3) pose-graph optimisation on the device (include/aria_orb_hip.h, "SE(3) pose-graph optimisation"): what the reference's
PoseGraphOptimizer (include/legacy/LoopClosure.hpp:80-113, src/legacy/LoopClosure.cpp:197-312) asks of g2o, batched over
graphs. aria_slam_amd.graph_ref restates the stage in NumPy and is its definition.

HipPoseGraphOptimizer carries the reference class's surface (set_initial_pose, add_odometry_edge, add_loop_edge, optimize,
get_optimized_pose, get_all_poses, clear) with the bookkeeping of graph_ref.PoseGraph, plus optimize_batch (host graphs) and
optimize_batch_device (device pointers).

As with HipFundamentalEstimator, the handle's own stream is non-blocking: device buffers filled on torch's default stream
must be synchronised before optimize_batch_device, or the optimizer must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import GRAPH_EDGE_DTYPE, GRAPH_RESULT_DTYPE, check
from .frontend import _ptr
from .graph_ref import PoseGraph


def pack_poses(poses):
    """(V, 4, 4) or (V, 3, 4) -> contiguous (V, 12) float64, the rows of [R t]."""
    p = np.asarray(poses, np.float64)
    p = p.reshape(-1, p.shape[-2], 4)[:, :3, :] if p.size else p.reshape(0, 3, 4)
    return np.ascontiguousarray(p).reshape(-1, 12).copy()


def unpack_poses(rows):
    """(V, 12) -> (V, 4, 4)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 3, 4)
    out = np.zeros((len(rows), 4, 4))
    out[:, :3, :] = rows
    out[:, 3, 3] = 1.0
    return out


def pack_edges(edges):
    """[(from, to, info_scale, Z 4x4)] -> GRAPH_EDGE_DTYPE records."""
    rec = np.zeros(len(edges), GRAPH_EDGE_DTYPE)
    for k, (i, j, s, Z) in enumerate(edges):
        rec[k] = (i, j, s, np.asarray(Z, np.float64).reshape(-1, 4)[:3].reshape(12))
    return rec


def _result_dict(rec):
    r = {k: (float(rec[k]) if k in ("chi2_initial", "chi2_final", "lambda") else int(rec[k]))
         for k in GRAPH_RESULT_DTYPE.names if k != "reserved"}
    r["lambda_"] = r.pop("lambda")
    r["record"] = rec.tobytes()          # the raw aria_graph_result (48 bytes)
    return r


class HipPoseGraphOptimizer(StageHandle, PoseGraph):
    """Binding of aria_graph_t behind the reference class's methods. The first vertex added is the fixed one; loop edges
    carry 10x the information; edges that name an unknown id are dropped."""

    _prefix, _config = "graph", _lib.GraphConfig

    def __init__(self, max_vertices=4096, max_edges=8192, max_graphs=1, pcg_max_iters=1000, pcg_rel_tol=1e-8, stream=None,
                 device=0):
        super().__init__()
        cfg = self._default_config(device, stream)
        cfg.max_graphs, cfg.max_vertices, cfg.max_edges = max_graphs, max_vertices, max_edges
        cfg.pcg_max_iters, cfg.pcg_rel_tol = pcg_max_iters, pcg_rel_tol
        self._create(cfg)
        self.last_result = None

    # ---- the reference class's optimize(): the graph held by this object
    def optimize(self, iterations=10):
        if not self.poses:
            return
        out, self.last_result = self.optimize_graph(np.array(self.poses), self.edges, 0, iterations)
        self.poses = [p for p in out]

    # ---- arrays
    def optimize_graph(self, poses, edges, fixed=0, iterations=10):
        """One graph, host arrays: poses (V, 4, 4), edges [(from, to, info_scale, Z 4x4)] or GRAPH_EDGE_DTYPE records.
        Returns (poses (V, 4, 4), dict of the aria_graph_result fields)."""
        rows = pack_poses(poses)
        rec = edges if isinstance(edges, np.ndarray) and edges.dtype == GRAPH_EDGE_DTYPE else pack_edges(edges)
        rec = np.ascontiguousarray(rec)
        res = np.zeros(1, GRAPH_RESULT_DTYPE)
        check(self._L.aria_graph_optimize(self._h, rows.ctypes.data if len(rows) else None, len(rows), fixed,
                                          rec.ctypes.data if len(rec) else None, len(rec), iterations, res.ctypes.data),
              "aria_graph_optimize")
        return unpack_poses(rows), _result_dict(res[0])

    def optimize_batch(self, graphs, iterations=10, raise_on_error=True):
        """graphs: [(poses (V, 4, 4), edges, fixed)]. One aria_graph_optimize_batch_device call over all of them. Returns
        ([poses (V, 4, 4)], [result dict], status of aria_graph_check); raises on a deferred error unless told not to."""
        import torch

        B = len(graphs)
        if B == 0:
            return [], [], 0
        rows = [pack_poses(g[0]) for g in graphs]
        recs = [g[1] if isinstance(g[1], np.ndarray) and g[1].dtype == GRAPH_EDGE_DTYPE else pack_edges(g[1]) for g in graphs]
        voff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        eoff = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
        fixed = np.array([g[2] for g in graphs], np.int32)
        allrows = np.concatenate(rows + [np.zeros((1, 12))])          # never empty
        allrecs = np.concatenate(recs + [np.zeros(1, GRAPH_EDGE_DTYPE)])
        dev = torch.device("cuda", self.config.device)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
        dp, dv, de, do, df = d(allrows), d(voff), d(allrecs), d(eoff), d(fixed)
        dres = torch.zeros(B * GRAPH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)          # the handle's own stream is not ordered against torch's default stream
        self.optimize_batch_device(dp, dv, de, do, df, B, iterations, dres)
        status = self.status()
        if status != 0 and raise_on_error:
            check(status, "aria_graph_check")
        out = np.frombuffer(dp.cpu().numpy().tobytes(), np.float64).reshape(-1, 12)
        res = np.frombuffer(dres.cpu().numpy().tobytes(), GRAPH_RESULT_DTYPE)
        poses = [unpack_poses(out[voff[g]:voff[g + 1]]) for g in range(B)]
        return poses, [_result_dict(res[g]) for g in range(B)], status

    def optimize_batch_device(self, d_poses, d_vertex_offset, d_edges, d_edge_offset, d_fixed, n_graphs, iterations, d_results):
        """aria_graph_optimize_batch_device: device pointers (torch tensors or ints). d_poses: 12 doubles per vertex, updated
        in place; d_results: n_graphs * 48 bytes (GRAPH_RESULT_DTYPE). Enqueued on the handle's stream; check()
        synchronises."""
        check(self._L.aria_graph_optimize_batch_device(self._h, _ptr(d_poses), _ptr(d_vertex_offset), _ptr(d_edges),
                                                       _ptr(d_edge_offset), _ptr(d_fixed), n_graphs, iterations,
                                                       _ptr(d_results)), "aria_graph_optimize_batch_device")

    def debug_linearize(self, poses, edges, fixed=0):
        """(chi2, b (V, 6), H_diag (V, 6, 6), H_off (E, 6, 6)) of one graph at its poses."""
        rows, rec = pack_poses(poses), np.ascontiguousarray(pack_edges(edges))
        V, E = len(rows), len(rec)
        chi2 = C.c_double()
        b, D, W = np.zeros((max(V, 1), 6)), np.zeros((max(V, 1), 6, 6)), np.zeros((max(E, 1), 6, 6))
        check(self._L.aria_graph_debug_linearize(self._h, rows.ctypes.data if V else None, V, fixed,
                                                 rec.ctypes.data if E else None, E, C.byref(chi2), b.ctypes.data,
                                                 D.ctypes.data, W.ctypes.data), "aria_graph_debug_linearize")
        return chi2.value, b[:V], D[:V], W[:E]
