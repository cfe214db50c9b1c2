"""Loop alignment on the device (include/aria_orb_hip.h, "loop alignment"): the similarity X2 = s R X1 + t between the
landmarks two keyframes of a loop own -- Sim(3) RANSAC over three-point closed forms, two-sided fp32 reprojection scoring,
Gauss-Newton refinement -- and the join of a match list with the point map that produces the correspondences.
aria_slam_amd.sim3_ref restates the stage in NumPy and is its definition; the reference project has no code for it.

The handle's own stream is non-blocking: it is not ordered against the legacy default stream, where torch works unless told
otherwise. Device buffers filled there must be synchronised (torch.cuda.synchronize()) before the device calls, or the
aligner must be created on the caller's stream."""

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import SIM3_CORR_DTYPE, SIM3_RESULT_DTYPE, check
from .frontend import _ptr


def _result_dict(rec, mask=None):
    r = dict(R=rec["R"].reshape(3, 3).copy(), t=rec["t"].copy(), s=float(rec["s"]), rms_px=float(rec["rms_px"]))
    for k in ("n_corr", "n_inliers", "best_hypothesis", "iterations", "refined", "valid"):
        r[k] = int(rec[k])
    r["record"] = rec.tobytes()          # the raw aria_sim3_result (136 bytes)
    if mask is not None:
        r["mask"] = mask
    return r


def _corr(corr):
    c = np.ascontiguousarray(corr)
    if c.dtype != SIM3_CORR_DTYPE:
        c = c.view(SIM3_CORR_DTYPE)
    return c.reshape(-1)


class HipSim3Aligner(StageHandle):
    """Binding of aria_sim3_t. K = (fx, fy, cx, cy); the defaults are EuRoC cam0 and 3 px (ORB-SLAM's bound at octave 0,
    untuned). fix_scale=1: s = 1 everywhere, for a metric stereo map."""

    _prefix, _config = "sim3", _lib.Sim3Config

    def __init__(self, K=None, hypotheses=1024, threshold_px=3.0, refine_iters=5, fix_scale=0, min_scale=0.05, max_scale=20.0,
                 seed=0, stream=None, device=0):
        cfg = self._default_config(device, stream)
        cfg.hypotheses = hypotheses
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.threshold_px = threshold_px
        cfg.refine_iters = refine_iters
        cfg.fix_scale = fix_scale
        cfg.min_scale, cfg.max_scale = min_scale, max_scale
        cfg.seed = seed
        self._create(cfg)

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    def estimate(self, corr, pair_base=0):
        """One pair, a host array of SIM3_CORR_DTYPE (X1, X2, u1, v1, u2, v2). Returns a dict of the aria_sim3_result fields
        (R 3x3, t, s, rms_px, counts, valid) and `mask` (uint8 per correspondence). A pair with a value that is not finite
        raises (ARIA_E_INVALID) after the call has run."""
        c = _corr(corr)
        rec = np.zeros(1, SIM3_RESULT_DTYPE)
        mask = np.zeros(max(len(c), 1), np.uint8)
        check(self._L.aria_sim3_estimate(self._h, c.ctypes.data if len(c) else None, len(c), pair_base, rec.ctypes.data,
                                         mask.ctypes.data), "aria_sim3_estimate")
        return _result_dict(rec[0], mask[:len(c)])

    def estimate_batch_device(self, d_corr, d_ncorr, n_pairs, corr_cap, d_out, d_mask=None, pair_base=0):
        """aria_sim3_estimate_batch_device: device pointers (torch tensors or ints); d_out holds n_pairs * 136 bytes
        (SIM3_RESULT_DTYPE records). Enqueued on the handle's stream; check() synchronises and reports deferred errors."""
        check(self._L.aria_sim3_estimate_batch_device(self._h, _ptr(d_corr), _ptr(d_ncorr), n_pairs, corr_cap, pair_base,
                                                      _ptr(d_out), _ptr(d_mask)), "aria_sim3_estimate_batch_device")

    def associate_batch_device(self, mapper, d_anchor1, d_anchor2, view1, view2, d_pose1, d_pose2, d_kp1, d_n1, d_kp2, d_n2,
                               kp_stride, d_matches, d_nmatches, n_pairs, match_cap, d_corr, d_ncorr, d_corr_match=None):
        """aria_sim3_associate_batch_device: the correspondences of n_pairs match lists (query = keyframe 1, train =
        keyframe 2) against the points of `mapper` (a HipMapper) that the two keyframes own (pair == d_anchorJ[p], indexed by
        idx{viewJ}), moved into the cameras by the 12-double poses at d_poseJ + 12 p; written at d_corr + p * match_cap
        (64 bytes each). Enqueued."""
        check(self._L.aria_sim3_associate_batch_device(self._h, mapper._h, _ptr(d_anchor1), _ptr(d_anchor2), view1, view2,
                                                       _ptr(d_pose1), _ptr(d_pose2), _ptr(d_kp1), _ptr(d_n1), _ptr(d_kp2),
                                                       _ptr(d_n2), kp_stride, _ptr(d_matches), _ptr(d_nmatches), n_pairs,
                                                       match_cap, _ptr(d_corr), _ptr(d_ncorr), _ptr(d_corr_match)),
              "aria_sim3_associate_batch_device")

    def debug_hypotheses(self, corr, pair_base=0):
        """(sample_idx (H, 3) int32, R (H, 9) float32, t (H, 3) float32, s (H,) float32, counts (H,) int32) of one pair --
        the test hook."""
        c = _corr(corr)
        H = self.config.hypotheses
        idx = np.zeros((H, 3), np.int32)
        R = np.zeros((H, 9), np.float32)
        t = np.zeros((H, 3), np.float32)
        s = np.zeros(H, np.float32)
        cnt = np.zeros(H, np.int32)
        check(self._L.aria_sim3_debug_hypotheses(self._h, c.ctypes.data if len(c) else None, len(c), pair_base, idx.ctypes.data,
                                                 R.ctypes.data, t.ctypes.data, s.ctypes.data, cnt.ctypes.data),
              "aria_sim3_debug_hypotheses")
        return idx, R, t, s, cnt
