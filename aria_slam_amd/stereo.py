"""Sparse stereo on the device (include/aria_orb_hip.h, "sparse stereo"): a depth per left keypoint of a RECTIFIED stereo
pair and the metric scale of a relative pose. The reference has no stereo code; aria_slam_amd.stereo_ref is the definition
and the device equals it bit for bit. Rectification / undistortion is not part of the stage: see aria_rect_*
(aria_slam_amd.rectify.HipRectifier), whose output images and new K this stage takes.

As with HipPoseEstimator, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_batch_device call, or the matcher must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import KP_DTYPE, MATCH_DTYPE, POSE_RESULT_DTYPE, STEREO_OBS_DTYPE, STEREO_SCALE_DTYPE, check
from .frontend import _ptr


def _kps(frame_or_array):
    k = frame_or_array["keypoints"] if isinstance(frame_or_array, dict) else frame_or_array
    k = np.ascontiguousarray(k)
    if k.dtype != KP_DTYPE:
        k = k.view(KP_DTYPE)
    return k.reshape(-1)


def _addr(a):
    return a.ctypes.data if len(a) else None


class HipStereoMatcher(StageHandle):
    """Binding of aria_stereo_t. K = (fx, fy, cx, cy) of the rectified left camera (default EuRoC cam0); max_disparity
    defaults to fx (depth >= baseline)."""

    _prefix, _config = "stereo", _lib.StereoConfig

    def __init__(self, K=None, baseline=0.110, min_disparity=0.0, max_disparity=None, th_hamming=75, sad_half_window=5,
                 sad_slide=5, band_factor=2.0, max_octave_diff=1, median_factor=2.1, min_scale_matches=5, stream=None,
                 device=0):
        cfg = self._default_config(device, stream)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.baseline = baseline
        cfg.min_disparity = min_disparity
        cfg.max_disparity = cfg.fx if max_disparity is None else max_disparity
        cfg.th_hamming, cfg.sad_half_window, cfg.sad_slide = th_hamming, sad_half_window, sad_slide
        cfg.band_factor, cfg.max_octave_diff, cfg.median_factor = band_factor, max_octave_diff, median_factor
        cfg.min_scale_matches = min_scale_matches
        self._create(cfg)

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    def match(self, img_left, img_right, left, right):
        """One rectified pair from host arrays; blocks. left / right: frame dicts of OrbHipExtractor.extract (keypoints,
        descriptors) or (keypoints, descriptors) tuples. Returns (obs: STEREO_OBS_DTYPE per left keypoint, matches:
        MATCH_DTYPE in ascending left index)."""
        il, ir = np.asarray(img_left, np.uint8), np.asarray(img_right, np.uint8)
        if il.ndim != 2 or il.shape != ir.shape:
            raise ValueError("the two images must be gray and of one size")
        if il.strides != ir.strides or il.strides[1] != 1 or il.strides[0] < il.shape[1]:   # one pitch serves both sides
            il, ir = np.ascontiguousarray(il), np.ascontiguousarray(ir)
        kl, dl = (left["keypoints"], left["descriptors"]) if isinstance(left, dict) else left
        kr, dr = (right["keypoints"], right["descriptors"]) if isinstance(right, dict) else right
        kl, kr = _kps(kl), _kps(kr)
        dl = np.ascontiguousarray(dl, np.uint8).reshape(-1, 32)
        dr = np.ascontiguousarray(dr, np.uint8).reshape(-1, 32)
        if len(dl) != len(kl) or len(dr) != len(kr):
            raise ValueError("one descriptor per keypoint")
        obs = np.zeros(max(len(kl), 1), STEREO_OBS_DTYPE)
        m = np.zeros(max(len(kl), 1), MATCH_DTYPE)
        n = C.c_int(0)
        check(self._L.aria_stereo_match(self._h, il.ctypes.data, ir.ctypes.data, il.shape[1], il.shape[0], il.strides[0],
                                        _addr(kl), _addr(dl), len(kl), _addr(kr), _addr(dr), len(kr), obs.ctypes.data,
                                        m.ctypes.data, C.byref(n)), "aria_stereo_match")
        return obs[:len(kl)], m[:n.value]

    def match_batch_device(self, d_img_left, d_img_right, img_stride, width, height, pitch, d_kp_left, d_desc_left, d_n_left,
                           d_kp_right, d_desc_right, d_n_right, kp_stride, n_pairs, d_obs, d_matches, d_nmatches,
                           match_cap=None):
        """aria_stereo_match_batch_device: device pointers (torch tensors or ints). d_obs holds n_pairs * kp_stride
        STEREO_OBS_DTYPE records, d_matches n_pairs * match_cap MATCH_DTYPE rows (match_cap defaults to kp_stride). Enqueued
        on the handle's stream; check() synchronises and reports deferred errors."""
        check(self._L.aria_stereo_match_batch_device(
            self._h, _ptr(d_img_left), _ptr(d_img_right), img_stride, width, height, pitch, _ptr(d_kp_left), _ptr(d_desc_left),
            _ptr(d_n_left), _ptr(d_kp_right), _ptr(d_desc_right), _ptr(d_n_right), kp_stride, n_pairs, _ptr(d_obs),
            _ptr(d_matches), _ptr(d_nmatches), kp_stride if match_cap is None else match_cap),
            "aria_stereo_match_batch_device")

    def scale(self, pose, matches, obs_query, obs_train, mask=None, query_is_first=True):
        """Metric scale of one relative pose from host arrays; blocks. pose: HipPoseEstimator.estimate's dict (its `mask` is
        used unless one is given) or a POSE_RESULT_DTYPE record. Returns a STEREO_SCALE_DTYPE record."""
        if isinstance(pose, dict):
            rec = np.frombuffer(pose["record"], POSE_RESULT_DTYPE).copy()
            if mask is None:
                mask = pose.get("mask")
        else:
            rec = np.ascontiguousarray(pose).view(POSE_RESULT_DTYPE).reshape(-1)[:1].copy()
        m = np.ascontiguousarray(matches)
        if len(m) and m.dtype != MATCH_DTYPE:
            m = m.view(MATCH_DTYPE)
        oq = np.ascontiguousarray(obs_query).view(STEREO_OBS_DTYPE).reshape(-1)
        ot = np.ascontiguousarray(obs_train).view(STEREO_OBS_DTYPE).reshape(-1)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mk is not None and len(mk) < len(m):
            raise ValueError("mask shorter than the match list")
        out = np.zeros(1, STEREO_SCALE_DTYPE)
        check(self._L.aria_stereo_scale_pose(self._h, rec.ctypes.data, None if mk is None or not len(mk) else mk.ctypes.data,
                                             _addr(m), len(m), 1 if query_is_first else 0, _addr(oq), len(oq), _addr(ot),
                                             len(ot), out.ctypes.data), "aria_stereo_scale_pose")
        return out[0]

    def scale_batch_device(self, d_pose, d_mask, d_matches, d_nmatches, match_cap, d_obs_query, d_nq, d_obs_train, d_nt,
                           kp_stride, n_pairs, d_out, query_is_first=True):
        """aria_stereo_scale_batch_device: device pointers (torch tensors or ints); d_out holds n_pairs STEREO_SCALE_DTYPE
        records."""
        check(self._L.aria_stereo_scale_batch_device(
            self._h, _ptr(d_pose), _ptr(d_mask), _ptr(d_matches), _ptr(d_nmatches), match_cap, 1 if query_is_first else 0,
            _ptr(d_obs_query), _ptr(d_nq), _ptr(d_obs_train), _ptr(d_nt), kp_stride, n_pairs, _ptr(d_out)),
            "aria_stereo_scale_batch_device")
