"""Absolute pose from the point map on the device (include/aria_orb_hip.h, "absolute pose from the point map"): PnP RANSAC over
3D-2D correspondences -- a 6-point DLT or a P3P minimal solver, fp32 reprojection scoring, Gauss-Newton refinement -- and the join of
a match list with the map that produces the correspondences. aria_slam_amd.pnp_ref restates the stage in NumPy and is its
definition; the reference project has no PnP code.

The handle's own stream is non-blocking: it is not ordered against the legacy default stream, where torch works unless told
otherwise. Device buffers filled there must be synchronised (torch.cuda.synchronize()) before the device calls, or the
estimator must be created on the caller's stream."""

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import PNP_CORR_DTYPE, PNP_RESULT_DTYPE, check
from .frontend import _ptr


def _result_dict(rec, mask=None):
    r = dict(R=rec["R"].reshape(3, 3).copy(), t=rec["t"].copy(), rms_px=float(rec["rms_px"]))
    for k in ("n_corr", "n_inliers", "best_hypothesis", "iterations", "refined", "valid"):
        r[k] = int(rec[k])
    r["record"] = rec.tobytes()          # the raw aria_pnp_result (128 bytes)
    if mask is not None:
        r["mask"] = mask
    return r


def _corr(corr):
    c = np.ascontiguousarray(corr)
    if c.dtype != PNP_CORR_DTYPE:
        c = c.view(PNP_CORR_DTYPE)
    return c.reshape(-1)


SOLVERS = {"dlt": 0, "p3p": 1}           # ARIA_PNP_SOLVER_DLT6, ARIA_PNP_SOLVER_P3P


class HipPnPEstimator(StageHandle):
    """Binding of aria_pnp_t. K = (fx, fy, cx, cy); the defaults are EuRoC cam0 and the map stage's 2 px. solver: "dlt" (the
    6-point DLT, which yields valid = 0 on a planar scene) or "p3p" (four correspondences are enough, planar scenes
    included); it can be changed between calls through the `solver` property."""

    _prefix, _config = "pnp", _lib.PnpConfig

    def __init__(self, K=None, hypotheses=1024, threshold_px=2.0, refine_iters=5, seed=0, stream=None, device=0, solver="dlt"):
        if solver not in SOLVERS:
            raise ValueError("solver must be one of %r" % (sorted(SOLVERS),))
        cfg = self._default_config(device, stream)
        cfg.hypotheses = hypotheses
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.threshold_px = threshold_px
        cfg.refine_iters = refine_iters
        cfg.seed = seed
        self._create(cfg)
        if solver != "dlt":
            self.solver = solver

    @property
    def solver(self):
        """The minimal solver of the calls issued from now on: "dlt" or "p3p" (aria_pnp_set_solver; nothing is synchronised)."""
        code = self._L.aria_pnp_get_solver(self._h)
        return [k for k, v in SOLVERS.items() if v == code][0]

    @solver.setter
    def solver(self, name):
        if name not in SOLVERS:
            raise ValueError("solver must be one of %r" % (sorted(SOLVERS),))
        check(self._L.aria_pnp_set_solver(self._h, SOLVERS[name]), "aria_pnp_set_solver")

    def set_solver_code(self, code):
        """aria_pnp_set_solver with a raw value; returns the status (an unknown value: ARIA_E_INVALID, nothing changes)."""
        return int(self._L.aria_pnp_set_solver(self._h, int(code)))

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    def estimate(self, corr, pair_base=0):
        """One pair, a host array of PNP_CORR_DTYPE (X, u, v). Returns a dict of the aria_pnp_result fields (R 3x3, t, rms_px,
        counts, valid) and `mask` (uint8 per correspondence)."""
        c = _corr(corr)
        rec = np.zeros(1, PNP_RESULT_DTYPE)
        mask = np.zeros(max(len(c), 1), np.uint8)
        check(self._L.aria_pnp_estimate(self._h, c.ctypes.data if len(c) else None, len(c), pair_base, rec.ctypes.data,
                                        mask.ctypes.data), "aria_pnp_estimate")
        return _result_dict(rec[0], mask[:len(c)])

    def estimate_batch_device(self, d_corr, d_ncorr, n_pairs, corr_cap, d_out, d_mask=None, pair_base=0):
        """aria_pnp_estimate_batch_device: device pointers (torch tensors or ints); d_out holds n_pairs * 128 bytes
        (PNP_RESULT_DTYPE records). Enqueued on the handle's stream; check() synchronises and reports deferred errors."""
        check(self._L.aria_pnp_estimate_batch_device(self._h, _ptr(d_corr), _ptr(d_ncorr), n_pairs, corr_cap, pair_base,
                                                     _ptr(d_out), _ptr(d_mask)), "aria_pnp_estimate_batch_device")

    def associate_batch_device(self, mapper, anchor_base, anchor_view, d_kp_query, d_nq, kp_stride, d_matches, d_nmatches,
                               n_pairs, match_cap, d_corr, d_ncorr, d_corr_match=None):
        """aria_pnp_associate_batch_device: the correspondences of n_pairs match lists against the points of `mapper` (a
        HipMapper) whose pair id is anchor_base + p, written at d_corr + p * match_cap (32 bytes each). Enqueued."""
        check(self._L.aria_pnp_associate_batch_device(self._h, mapper._h, anchor_base, anchor_view, _ptr(d_kp_query), _ptr(d_nq),
                                                      kp_stride, _ptr(d_matches), _ptr(d_nmatches), n_pairs, match_cap,
                                                      _ptr(d_corr), _ptr(d_ncorr), _ptr(d_corr_match)),
              "aria_pnp_associate_batch_device")

    def debug_hypotheses(self, corr, pair_base=0):
        """(sample_idx (H, 6) int32, R (H, 9) float32, t0 (H, 3) float32, counts (H,) int32) of one pair -- the test hook.
        With the P3P solver slots 4 and 5 of sample_idx are -1."""
        c = _corr(corr)
        H = self.config.hypotheses
        idx = np.zeros((H, 6), np.int32)
        R = np.zeros((H, 9), np.float32)
        t0 = np.zeros((H, 3), np.float32)
        cnt = np.zeros(H, np.int32)
        check(self._L.aria_pnp_debug_hypotheses(self._h, c.ctypes.data if len(c) else None, len(c), pair_base, idx.ctypes.data,
                                                R.ctypes.data, t0.ctypes.data, cnt.ctypes.data), "aria_pnp_debug_hypotheses")
        return idx, R, t0, cnt
