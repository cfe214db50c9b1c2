"""Guided matching on the device (include/aria_orb_hip.h, "guided matching"): landmarks projected into frames by a predicted
pose, the keypoints searched in a window around each projection, the matches as aria_pnp_corr for HipPnPEstimator. The
reference has no such code; aria_slam_amd.proj_ref is the definition and the device equals it bit for bit.

As with HipPoseEstimator, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_device call, or the matcher must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import KP_DTYPE, PNP_CORR_DTYPE, PROJ_LANDMARK_DTYPE, PROJ_OBS_DTYPE, PROJ_PAIR_DTYPE, check
from .frontend import _ptr


def _addr(a):
    return a.ctypes.data if len(a) else None


class HipProjectionMatcher(StageHandle):
    """Binding of aria_proj_t. K = (fx, fy, cx, cy) (default EuRoC cam0). radius_px, ratio, th_hamming and max_octave_diff
    default to ORB-SLAM's published tracking constants; nobody has tuned them on a recording here."""

    _prefix, _config = "proj", _lib.ProjConfig

    def __init__(self, K=None, min_depth=0.1, radius_px=15.0, ratio=0.9, th_hamming=100, max_octave_diff=1, stream=None,
                 device=0):
        cfg = self._default_config(device, stream)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.min_depth, cfg.radius_px, cfg.ratio = min_depth, radius_px, ratio
        cfg.th_hamming, cfg.max_octave_diff = th_hamming, max_octave_diff
        self._create(cfg)

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    def search(self, pose, keypoints, descriptors, landmarks, width, height):
        """One frame from host arrays, every landmark searched; blocks. pose: 12 doubles [R|t] row-major, world to camera.
        Returns (obs: PROJ_OBS_DTYPE per landmark, corr: PNP_CORR_DTYPE, pairs: PROJ_PAIR_DTYPE), the last two in ascending
        landmark index."""
        P = np.ascontiguousarray(pose, np.float64).reshape(-1)
        if len(P) != 12:
            raise ValueError("the pose is 12 doubles [R|t], row-major")
        k = np.ascontiguousarray(keypoints)
        if k.dtype != KP_DTYPE:
            k = k.view(KP_DTYPE)
        k = k.reshape(-1)
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        if len(d) != len(k):
            raise ValueError("one descriptor per keypoint")
        lm = np.ascontiguousarray(landmarks).view(PROJ_LANDMARK_DTYPE).reshape(-1)
        cap = max(len(lm), 1)
        obs, corr, pairs = np.zeros(cap, PROJ_OBS_DTYPE), np.zeros(cap, PNP_CORR_DTYPE), np.zeros(cap, PROJ_PAIR_DTYPE)
        n = C.c_int(0)
        check(self._L.aria_proj_search(self._h, P.ctypes.data, _addr(k), _addr(d), len(k), width, height, _addr(lm), len(lm),
                                       obs.ctypes.data, corr.ctypes.data, pairs.ctypes.data, C.byref(n)), "aria_proj_search")
        return obs[:len(lm)], corr[:n.value], pairs[:n.value]

    def search_batch_device(self, d_pose, d_kp, d_desc, d_n, kp_stride, width, height, d_land, n_landmarks, d_range, land_cap,
                            n_frames, d_obs, d_corr, d_pairs, d_ncorr):
        """aria_proj_search_batch_device: device pointers (torch tensors or ints). Frame f reads 12 doubles at d_pose + 12 f,
        its keypoints and descriptors as the extractor's batch form leaves them, and the landmarks
        d_land[d_range[2f] : d_range[2f] + d_range[2f+1]]; d_obs holds n_frames * land_cap PROJ_OBS_DTYPE records, d_corr and
        d_pairs as many PNP_CORR_DTYPE / PROJ_PAIR_DTYPE records, d_ncorr n_frames ints. Enqueued on the handle's stream;
        check() synchronises and reports deferred errors."""
        check(self._L.aria_proj_search_batch_device(
            self._h, _ptr(d_pose), _ptr(d_kp), _ptr(d_desc), _ptr(d_n), kp_stride, width, height, _ptr(d_land), n_landmarks,
            _ptr(d_range), land_cap, n_frames, _ptr(d_obs), _ptr(d_corr), _ptr(d_pairs), _ptr(d_ncorr)),
            "aria_proj_search_batch_device")

    def landmarks_from_map_device(self, mapper, first, max_count, pair_base, view, d_kp, d_desc, d_n, kp_stride, n_slots, d_land,
                                  d_nland):
        """aria_proj_landmarks_from_map_device: arena positions [first, first + max_count) of `mapper` (a HipMapper) as
        max_count PROJ_LANDMARK_DTYPE records at d_land, their number at d_nland[0]; a point of pair p takes the descriptor
        and octave of keypoint idx1 (view 1) or idx2 (view 2) of slot p - pair_base. Enqueued."""
        check(self._L.aria_proj_landmarks_from_map_device(self._h, mapper._h, first, max_count, pair_base, view, _ptr(d_kp),
                                                          _ptr(d_desc), _ptr(d_n), kp_stride, n_slots, _ptr(d_land),
                                                          _ptr(d_nland)), "aria_proj_landmarks_from_map_device")
