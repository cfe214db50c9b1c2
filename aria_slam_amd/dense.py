"""Dense stereo on the device (include/aria_orb_hip.h, "dense stereo"): census + four-path semi-global matching over 64
disparities on RECTIFIED pairs, a disparity map in 1/16 px (int16, -16 = invalid), an fp32 depth map, and the stereo
observation at each keypoint in the sparse stage's record, so the scale call and the mapper take dense depths unchanged.
The reference has no code for it; aria_slam_amd.dense_ref is the definition and the device equals it bit for bit.
Rectification is aria_rect_* (aria_slam_amd.rectify.HipRectifier), whose output images and new K this stage takes.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_batch_device call, or the handle must be created on the caller's stream."""
import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import KP_DTYPE, STEREO_OBS_DTYPE, check
from .frontend import _ptr


class HipDenseStereo(StageHandle):
    """Binding of aria_dense_t. K = (fx, fy, cx, cy) of the rectified left camera (default EuRoC cam0). max_size =
    (width, height) of the largest pair; scratch_bytes is the HBM budget that decides how many pairs are in flight."""

    _prefix, _config = "dense", _lib.DenseConfig

    def __init__(self, K=None, baseline=0.110, P1=8, P2=32, uniqueness=10, lr_max_diff=1, max_size=(752, 480), scratch_bytes=None,
                 num_disparities=64, stream=None, device=0):
        cfg = self._default_config(device, stream)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.baseline = baseline
        cfg.num_disparities = num_disparities
        cfg.P1, cfg.P2, cfg.uniqueness, cfg.lr_max_diff = P1, P2, uniqueness, lr_max_diff
        cfg.max_width, cfg.max_height = max_size
        if scratch_bytes is not None:
            cfg.scratch_bytes = scratch_bytes
        self._create(cfg)

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    @property
    def pairs_in_flight(self):
        return self._L.aria_dense_pairs_in_flight(self._h)

    def compute(self, img_left, img_right, depth=True):
        """One rectified pair from host arrays; blocks. Returns (disparity int16 [H, W] in 1/16 px, depth fp32 [H, W]) or the
        disparity alone with depth=False."""
        il, ir = np.asarray(img_left, np.uint8), np.asarray(img_right, np.uint8)
        if il.ndim != 2 or il.shape != ir.shape:
            raise ValueError("the two images must be gray and of one size")
        if il.strides != ir.strides or il.strides[1] != 1 or il.strides[0] < il.shape[1]:   # one pitch serves both sides
            il, ir = np.ascontiguousarray(il), np.ascontiguousarray(ir)
        h, w = il.shape
        disp = np.empty((h, w), np.int16)
        z = np.empty((h, w), np.float32) if depth else None
        check(self._L.aria_dense_compute(self._h, il.ctypes.data, ir.ctypes.data, w, h, il.strides[0], disp.ctypes.data,
                                         z.ctypes.data if depth else None), "aria_dense_compute")
        return (disp, z) if depth else disp

    def compute_batch_device(self, d_left, d_right, width, height, n_pairs, d_disp, d_depth=None, img_stride=None, pitch=None,
                             disp_stride=None, disp_pitch=None, depth_stride=None, depth_pitch=None):
        """aria_dense_compute_batch_device: device pointers (torch tensors or ints). Pitches default to the width and strides
        to pitch * height; those of the outputs are in elements. Enqueued on the handle's stream; check() synchronises."""
        pitch = width if pitch is None else pitch
        disp_pitch = width if disp_pitch is None else disp_pitch
        depth_pitch = width if depth_pitch is None else depth_pitch
        img_stride = pitch * height if img_stride is None else img_stride
        disp_stride = disp_pitch * height if disp_stride is None else disp_stride
        depth_stride = depth_pitch * height if depth_stride is None else depth_stride
        check(self._L.aria_dense_compute_batch_device(self._h, _ptr(d_left), _ptr(d_right), img_stride, width, height, pitch,
                                                      n_pairs, _ptr(d_disp), disp_stride, disp_pitch, _ptr(d_depth), depth_stride,
                                                      depth_pitch), "aria_dense_compute_batch_device")

    def sample(self, disp, kps):
        """The stereo observations of one frame's keypoints (KP_DTYPE records or a frame dict of OrbHipExtractor.extract) on
        a host disparity map; blocks. Returns STEREO_OBS_DTYPE records."""
        d = np.asarray(disp, np.int16)
        if d.ndim != 2:
            raise ValueError("the disparity map must be 2-D")
        if d.strides[1] != 2 or d.strides[0] % 2 or d.strides[0] < 2 * d.shape[1]:
            d = np.ascontiguousarray(d)
        k = kps["keypoints"] if isinstance(kps, dict) else kps
        k = np.ascontiguousarray(k)
        if k.dtype != KP_DTYPE:
            k = k.view(KP_DTYPE)
        k = k.reshape(-1)
        obs = np.zeros(len(k), STEREO_OBS_DTYPE)
        if len(k):
            check(self._L.aria_dense_sample(self._h, d.ctypes.data, d.shape[1], d.shape[0], d.strides[0] // 2, k.ctypes.data,
                                            len(k), obs.ctypes.data), "aria_dense_sample")
        return obs

    def sample_batch_device(self, d_disp, width, height, d_kp, d_n, kp_stride, n_frames, d_obs, disp_stride=None, disp_pitch=None):
        """aria_dense_sample_batch_device: device pointers (torch tensors or ints); d_obs holds n_frames * kp_stride
        STEREO_OBS_DTYPE records. Enqueued on the handle's stream; check() synchronises and reports deferred errors."""
        disp_pitch = width if disp_pitch is None else disp_pitch
        disp_stride = disp_pitch * height if disp_stride is None else disp_stride
        check(self._L.aria_dense_sample_batch_device(self._h, _ptr(d_disp), disp_stride, disp_pitch, width, height, _ptr(d_kp),
                                                     _ptr(d_n), kp_stride, n_frames, _ptr(d_obs)), "aria_dense_sample_batch_device")


def scratch_bytes_per_pair(width, height):
    return _lib.load_library().aria_dense_scratch_bytes_per_pair(width, height)


def algorithmic_bytes(width, height):
    return _lib.load_library().aria_dense_algorithmic_bytes(width, height)
