"""Sim(3) pose-graph optimisation and the map correction after a loop, on the device (include/aria_orb_hip.h, "Sim(3)
pose-graph optimisation"): the roles of ORB-SLAM's OptimizeEssentialGraph and CorrectLoop, batched over graphs.
aria_slam_amd.sgraph_ref restates the stage in NumPy and is its definition.

HipSim3GraphOptimizer carries HipPoseGraphOptimizer's surface with the bookkeeping of sgraph_ref.Sim3Graph: vertices enter as
camera-to-world poses with s = 1, add_loop_edge takes the s of the alignment, get_optimized_scale returns what the graph made
of it. correct_map_device moves a HipMapper's arena by each pair's anchor keyframe; correct_points does the same to a host
array of MAP_POINT_DTYPE records.

The handle's own stream is non-blocking: device buffers filled on torch's default stream must be synchronised before the
*_device calls, or the optimizer must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import MAP_POINT_DTYPE, SGRAPH_EDGE_DTYPE, SGRAPH_RESULT_DTYPE, SGRAPH_STATS_DTYPE, SGRAPH_VERTEX_DTYPE, check
from .frontend import _ptr
from .posegraph import _result_dict
from .sgraph_ref import Sim3Graph, norm_edges


def pack_vertices(vertices):
    """(V, 13) rows (R row-major, t, s) -> SGRAPH_VERTEX_DTYPE records."""
    v = np.ascontiguousarray(np.asarray(vertices, np.float64).reshape(-1, 13))
    return v.view(SGRAPH_VERTEX_DTYPE).reshape(-1).copy()


def unpack_vertices(rec):
    """SGRAPH_VERTEX_DTYPE records -> (V, 13)."""
    return np.ascontiguousarray(rec).view(np.float64).reshape(-1, 13).copy()


def pack_sim3_edges(edges):
    """[(from, to, info_scale, Z 4x4 or 3x4, s)] -> SGRAPH_EDGE_DTYPE records (s = 1 when an edge has four fields)."""
    if isinstance(edges, np.ndarray) and edges.dtype == SGRAPH_EDGE_DTYPE:
        return np.ascontiguousarray(edges)
    rec = np.zeros(len(edges), SGRAPH_EDGE_DTYPE)
    for k, (i, j, w, Z, s) in enumerate(norm_edges(edges)):
        rec[k] = (i, j, w, Z.reshape(12), s)
    return rec


def _dev_bytes(torch, dev, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)


class HipSim3GraphOptimizer(StageHandle, Sim3Graph):
    """Binding of aria_sgraph_t. The first vertex added is the fixed one; loop edges carry 10x the information and the scale
    of the alignment; edges that name an unknown id are dropped."""

    _prefix, _config = "sgraph", _lib.SgraphConfig

    def __init__(self, max_vertices=4096, max_edges=8192, max_graphs=1, pcg_max_iters=1000, pcg_rel_tol=1e-8, fix_scale=False,
                 stream=None, device=0):
        StageHandle.__init__(self)
        Sim3Graph.__init__(self)
        cfg = self._default_config(device, stream)
        cfg.max_graphs, cfg.max_vertices, cfg.max_edges = max_graphs, max_vertices, max_edges
        cfg.pcg_max_iters, cfg.pcg_rel_tol, cfg.fix_scale = pcg_max_iters, pcg_rel_tol, int(bool(fix_scale))
        self._create(cfg)
        self.last_result = None

    # ---- the graph held by this object
    def optimize(self, iterations=10):
        if not self.poses:
            return
        out, self.last_result = self.optimize_graph(self.vertices(), self.edges, 0, iterations)
        self._store(out)

    # ---- arrays
    def optimize_graph(self, vertices, edges, fixed=0, iterations=10):
        """One graph, host arrays: vertices (V, 13), edges [(from, to, info_scale, Z, s)] or SGRAPH_EDGE_DTYPE records.
        Returns (vertices (V, 13), dict of the aria_sgraph_result fields)."""
        vr, rec = pack_vertices(vertices), pack_sim3_edges(edges)
        res = np.zeros(1, SGRAPH_RESULT_DTYPE)
        check(self._L.aria_sgraph_optimize(self._h, vr.ctypes.data if len(vr) else None, len(vr), fixed,
                                           rec.ctypes.data if len(rec) else None, len(rec), iterations, res.ctypes.data),
              "aria_sgraph_optimize")
        return unpack_vertices(vr), _result_dict(res[0])

    def optimize_batch(self, graphs, iterations=10, raise_on_error=True):
        """graphs: [(vertices (V, 13), edges, fixed)]. One aria_sgraph_optimize_batch_device call over all of them. Returns
        ([vertices (V, 13)], [result dict], status of aria_sgraph_check); raises on a deferred error unless told not to."""
        import torch

        B = len(graphs)
        if B == 0:
            return [], [], 0
        rows = [pack_vertices(g[0]) for g in graphs]
        recs = [pack_sim3_edges(g[1]) for g in graphs]
        voff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        eoff = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
        fixed = np.array([g[2] for g in graphs], np.int32)
        allrows = np.concatenate(rows + [np.zeros(1, SGRAPH_VERTEX_DTYPE)])          # never empty
        allrecs = np.concatenate(recs + [np.zeros(1, SGRAPH_EDGE_DTYPE)])
        dev = torch.device("cuda", self.config.device)
        dp, dv, de, do, df = (_dev_bytes(torch, dev, x) for x in (allrows, voff, allrecs, eoff, fixed))
        dres = torch.zeros(B * SGRAPH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)          # the handle's own stream is not ordered against torch's default stream
        self.optimize_batch_device(dp, dv, de, do, df, B, iterations, dres)
        status = self.status()
        if status != 0 and raise_on_error:
            check(status, "aria_sgraph_check")
        out = np.frombuffer(dp.cpu().numpy().tobytes(), np.float64).reshape(-1, 13)
        res = np.frombuffer(dres.cpu().numpy().tobytes(), SGRAPH_RESULT_DTYPE)
        return [out[voff[g]:voff[g + 1]].copy() for g in range(B)], [_result_dict(res[g]) for g in range(B)], status

    def optimize_batch_device(self, d_vertices, d_vertex_offset, d_edges, d_edge_offset, d_fixed, n_graphs, iterations, d_results):
        """aria_sgraph_optimize_batch_device: device pointers (torch tensors or ints). d_vertices: 13 doubles per vertex,
        updated in place; d_results: n_graphs * 48 bytes. Enqueued on the handle's stream; check() synchronises."""
        check(self._L.aria_sgraph_optimize_batch_device(self._h, _ptr(d_vertices), _ptr(d_vertex_offset), _ptr(d_edges),
                                                        _ptr(d_edge_offset), _ptr(d_fixed), n_graphs, iterations,
                                                        _ptr(d_results)), "aria_sgraph_optimize_batch_device")

    def debug_linearize(self, vertices, edges, fixed=0):
        """(chi2, b (V, 7), H_diag (V, 7, 7), H_off (E, 7, 7)) of one graph at its vertices."""
        vr, rec = pack_vertices(vertices), pack_sim3_edges(edges)
        V, E = len(vr), len(rec)
        chi2 = C.c_double()
        b, D, W = np.zeros((max(V, 1), 7)), np.zeros((max(V, 1), 7, 7)), np.zeros((max(E, 1), 7, 7))
        check(self._L.aria_sgraph_debug_linearize(self._h, vr.ctypes.data if V else None, V, fixed,
                                                  rec.ctypes.data if E else None, E, C.byref(chi2), b.ctypes.data,
                                                  D.ctypes.data, W.ctypes.data), "aria_sgraph_debug_linearize")
        return chi2.value, b[:V], D[:V], W[:E]

    # ---- pose rows <-> vertices
    def vertices_from_pose_device(self, d_poses, d_vertices, n):
        check(self._L.aria_sgraph_vertices_from_pose_device(self._h, _ptr(d_poses), _ptr(d_vertices), n),
              "aria_sgraph_vertices_from_pose_device")

    def poses_from_vertices_device(self, d_vertices, d_poses, n):
        check(self._L.aria_sgraph_poses_from_vertices_device(self._h, _ptr(d_vertices), _ptr(d_poses), n),
              "aria_sgraph_poses_from_vertices_device")

    # ---- the map after a loop
    def correct_map_device(self, mapper, d_pair_vertex, n_table, pair_base, d_old, d_new, n_vertices, d_stats=None):
        """aria_sgraph_correct_map_device on a HipMapper's arena; device pointers. Enqueued on this handle's stream."""
        check(self._L.aria_sgraph_correct_map_device(self._h, mapper._h, _ptr(d_pair_vertex), n_table, pair_base, _ptr(d_old),
                                                     _ptr(d_new), n_vertices, _ptr(d_stats)), "aria_sgraph_correct_map_device")

    def correct_points_device(self, d_points, n_points, d_pair_vertex, n_table, pair_base, d_old, d_new, n_vertices, d_stats=None):
        check(self._L.aria_sgraph_correct_points_device(self._h, _ptr(d_points), n_points, _ptr(d_pair_vertex), n_table, pair_base,
                                                        _ptr(d_old), _ptr(d_new), n_vertices, _ptr(d_stats)),
              "aria_sgraph_correct_points_device")

    def _upload_correction(self, pair_vertex, old, new):
        import torch
        dev = torch.device("cuda", self.config.device)
        table = np.asarray(pair_vertex, np.int32).reshape(-1)
        vo, vn = pack_vertices(old), pack_vertices(new)
        assert len(vo) == len(vn)
        pad = lambda x, dt: x if len(x) else np.zeros(1, dt)      # noqa: E731
        d = [_dev_bytes(torch, dev, pad(x, dt)) for x, dt in ((table, np.int32), (vo, SGRAPH_VERTEX_DTYPE), (vn, SGRAPH_VERTEX_DTYPE))]
        dstats = torch.zeros(SGRAPH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        return torch, dev, d, len(table), len(vo), dstats

    @staticmethod
    def _stats(dstats):
        s = np.frombuffer(dstats.cpu().numpy().tobytes(), SGRAPH_STATS_DTYPE)[0]
        return int(s["moved"]), int(s["left_alone"]), int(s["refused"])

    def correct_map(self, mapper, pair_vertex, pair_base, old, new, raise_on_error=True):
        """Host tables and vertices ((V, 13) each) against a HipMapper's arena. Returns ((moved, left alone, refused), status)."""
        torch, dev, (dt, do, dn), n_table, nv, dstats = self._upload_correction(pair_vertex, old, new)
        torch.cuda.synchronize(dev)
        mapper.check()                       # the map's own stream has finished writing the arena
        self.correct_map_device(mapper, dt, n_table, pair_base, do, dn, nv, dstats)
        status = self.status()
        if status != 0 and raise_on_error:
            check(status, "aria_sgraph_check")
        return self._stats(dstats), status

    def correct_points(self, points, pair_vertex, pair_base, old, new, raise_on_error=True):
        """sgraph_ref.correct_points on the device: a host array of MAP_POINT_DTYPE records. Returns (points, (moved, left
        alone, refused), status)."""
        points = np.ascontiguousarray(points, MAP_POINT_DTYPE)
        torch, dev, (dt, do, dn), n_table, nv, dstats = self._upload_correction(pair_vertex, old, new)
        dp = _dev_bytes(torch, dev, points if len(points) else np.zeros(1, MAP_POINT_DTYPE))
        torch.cuda.synchronize(dev)
        self.correct_points_device(dp, len(points), dt, n_table, pair_base, do, dn, nv, dstats)
        status = self.status()
        if status != 0 and raise_on_error:
            check(status, "aria_sgraph_check")
        out = np.frombuffer(dp.cpu().numpy().tobytes(), MAP_POINT_DTYPE)[:len(points)].copy()
        return out, self._stats(dstats), status
