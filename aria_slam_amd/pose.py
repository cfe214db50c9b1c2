"""Two-view relative pose on the device (include/aria_orb_hip.h, "two-view relative pose"): essential-matrix RANSAC and
recoverPose -- what the reference does with every match list (cv::findEssentialMat(pts1, pts2, K, RANSAC, 0.999, 1.0) +
cv::recoverPose, src/euroc_eval.cpp:178-201). aria_slam_amd.pose_ref restates the stage in NumPy.

The handle's own stream is non-blocking: it is not ordered against the legacy default stream, where torch works unless told
otherwise. Device buffers filled there must be synchronised (torch.cuda.synchronize()) before estimate_batch_device, or
the estimator must be created on the caller's stream."""

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import KP_DTYPE, MATCH_DTYPE, POSE_RESULT_DTYPE, check
from .frontend import _ptr


def _result_dict(rec, mask=None):
    r = dict(R=rec["R"].reshape(3, 3).copy(), t=rec["t"].copy(), E=rec["E"].reshape(3, 3).copy())
    for k in ("n_matches", "n_inliers", "n_pose_inliers", "best_hypothesis", "refined", "valid"):
        r[k] = int(rec[k])
    r["record"] = rec.tobytes()          # the raw aria_pose_result (192 bytes)
    if mask is not None:
        r["mask"] = mask
    return r


def _kps(frame_or_array):
    k = frame_or_array["keypoints"] if isinstance(frame_or_array, dict) else frame_or_array
    k = np.ascontiguousarray(k)
    if k.dtype != KP_DTYPE:
        k = k.view(KP_DTYPE)
    return k


class HipPoseEstimator(StageHandle):
    """Binding of aria_pose_t. K = (fx, fy, cx, cy); defaults are EuRoC cam0 and OpenCV's findEssentialMat / recoverPose."""

    _prefix, _config = "pose", _lib.PoseConfig

    def __init__(self, K=None, hypotheses=1024, threshold_px=1.0, distance_thresh=50.0, seed=0, stream=None, device=0):
        cfg = self._default_config(device, stream)
        cfg.hypotheses = hypotheses
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.threshold_px = threshold_px
        cfg.distance_thresh = distance_thresh
        cfg.seed = seed
        self._create(cfg)

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    def estimate(self, kp1, kp2, matches, query_is_first=True, pair_base=0):
        """One pair, host arrays: kp1 = the query keypoints (frame dict or KP_DTYPE array), kp2 = the train keypoints,
        matches (MATCH_DTYPE). query_is_first: view 1 is the query side. Returns a dict of the aria_pose_result fields
        (R 3x3, t, E 3x3, counts, valid) and `mask` (uint8 per match)."""
        kq, kt = _kps(kp1), _kps(kp2)
        m = np.ascontiguousarray(matches)
        if len(m) and m.dtype != MATCH_DTYPE:
            m = m.view(MATCH_DTYPE)
        rec = np.zeros(1, POSE_RESULT_DTYPE)
        mask = np.zeros(max(len(m), 1), np.uint8)
        check(self._L.aria_pose_estimate(self._h, kq.ctypes.data if len(kq) else None, len(kq),
                                         kt.ctypes.data if len(kt) else None, len(kt), m.ctypes.data if len(m) else None,
                                         len(m), 1 if query_is_first else 0, pair_base, rec.ctypes.data, mask.ctypes.data),
              "aria_pose_estimate")
        return _result_dict(rec[0], mask[:len(m)])

    def estimate_batch_device(self, d_kp_query, d_nq, d_kp_train, d_nt, kp_stride, d_matches, d_nmatches, n_pairs, match_cap,
                              d_out, d_mask=None, query_is_first=True, pair_base=0):
        """aria_pose_estimate_batch_device: device pointers (torch tensors or ints); d_out holds n_pairs * 192 bytes
        (POSE_RESULT_DTYPE records). Enqueued on the handle's stream; check() synchronises and reports deferred errors."""
        check(self._L.aria_pose_estimate_batch_device(self._h, _ptr(d_kp_query), _ptr(d_nq), _ptr(d_kp_train), _ptr(d_nt),
                                                      kp_stride, _ptr(d_matches), _ptr(d_nmatches), n_pairs, match_cap,
                                                      1 if query_is_first else 0, pair_base, _ptr(d_out), _ptr(d_mask)),
              "aria_pose_estimate_batch_device")

    def debug_hypotheses(self, kp1, kp2, matches, query_is_first=True, pair_base=0):
        """(sample_idx (H, 8) int32, E (H, 9) float32, counts (H,) int32) of one pair -- the test hook."""
        kq, kt = _kps(kp1), _kps(kp2)
        m = np.ascontiguousarray(matches)
        if len(m) and m.dtype != MATCH_DTYPE:
            m = m.view(MATCH_DTYPE)
        H = self.config.hypotheses
        idx = np.zeros((H, 8), np.int32)
        E = np.zeros((H, 9), np.float32)
        cnt = np.zeros(H, np.int32)
        check(self._L.aria_pose_debug_hypotheses(self._h, kq.ctypes.data if len(kq) else None, len(kq),
                                                 kt.ctypes.data if len(kt) else None, len(kt),
                                                 m.ctypes.data if len(m) else None, len(m), 1 if query_is_first else 0,
                                                 pair_base, idx.ctypes.data, E.ctypes.data, cnt.ctypes.data),
              "aria_pose_debug_hypotheses")
        return idx, E, cnt
