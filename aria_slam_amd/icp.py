"""Frame-to-model tracking on the device (include/aria_orb_hip.h, "frame-to-model tracking"): batched point-to-plane ICP of
live fp32 depth maps against the depth maps and world-frame normals a HipVolumeRenderer predicted from the volume. The
reference has no code for it; aria_slam_amd.icp_ref is the definition and the device equals it bit for bit.

As with the other stages, the handle's own stream is non-blocking: maps written on another stream (the renderer's own) must
be synchronised before a call, or the tracker must be created on that stream."""
import numpy as np

from . import _lib, icp_ref
from ._handle import StageHandle
from ._lib import ICP_RESULT_DTYPE, ICP_TERMS, check
from .frontend import _ptr


class HipDenseTracker(StageHandle):
    """Binding of aria_icp_t. K = (fx, fy, cx, cy) of the live and the model maps (default EuRoC cam0); strides and iterations
    per level (default (4, 2, 1) and (4, 5, 10)); the other fields as aria_icp_config names them."""

    _prefix, _config = "icp", _lib.IcpConfig

    def __init__(self, K=None, min_depth=None, max_depth=None, dist_max=None, reach=None, min_corr=None, min_pivot=None, eps=None,
                 strides=None, iterations=None, stream=None, device=0):
        cfg = self._default_config(device, stream)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        for name, v in (("min_depth", min_depth), ("max_depth", max_depth), ("dist_max", dist_max), ("reach", reach),
                        ("min_corr", min_corr), ("min_pivot", min_pivot), ("eps", eps)):
            if v is not None:
                setattr(cfg, name, v)
        if (strides is None) != (iterations is None) or (strides is not None and not 1 <= len(strides) == len(iterations) <= 4):
            raise ValueError("strides and iterations are given together, one entry per level, at most 4 levels")
        if strides is not None:
            cfg.n_levels = len(strides)
            for l in range(4):
                cfg.stride[l] = int(strides[l]) if l < len(strides) else 0
                cfg.iterations[l] = int(iterations[l]) if l < len(strides) else 0
        self._create(cfg)

    @classmethod
    def from_renderer(cls, renderer, K, **kw):
        """A tracker for the views of a HipVolumeRenderer, on its device. K = (fx, fy, cx, cy) of the live maps: a renderer
        that casts with other intrinsics is refused, as both bindings refuse a volume of another geometry."""
        c = renderer.config
        if tuple(float(v) for v in K) != (c.fx, c.fy, c.cx, c.cy):
            raise ValueError("the renderer casts with other intrinsics than the tracker's")
        d = dict(K=K, device=c.device)
        d.update(kw)
        return cls(**d)

    @classmethod
    def from_ref_config(cls, cfg, **kw):
        return cls(K=cfg.K, min_depth=cfg.min_depth, max_depth=cfg.max_depth, dist_max=cfg.dist_max, reach=cfg.reach,
                   min_corr=cfg.min_corr, min_pivot=cfg.min_pivot, eps=cfg.eps, strides=cfg.strides, iterations=cfg.iterations, **kw)

    @property
    def ref_config(self):
        """The configuration as icp_ref.Config."""
        c = self.config
        return icp_ref.config(K=(c.fx, c.fy, c.cx, c.cy), min_depth=c.min_depth, max_depth=c.max_depth, dist_max=c.dist_max,
                              reach=c.reach, min_corr=c.min_corr, min_pivot=c.min_pivot, eps=c.eps,
                              strides=tuple(c.stride[:c.n_levels]), iterations=tuple(c.iterations[:c.n_levels]))

    @staticmethod
    def _layout(width, height, stride, pitch, per):
        pitch = width if pitch is None else pitch
        return (per * pitch * height if stride is None else stride), pitch

    def track_batch_device(self, d_depth, d_model_depth, d_model_normal, d_model_extrinsics, d_guess, n_frames, width, height,
                           d_extrinsics_out=None, d_results=None, d_mask=None, depth_stride=None, depth_pitch=None,
                           model_depth_stride=None, model_depth_pitch=None, normal_stride=None, normal_pitch=None):
        """aria_icp_track_batch_device: device pointers (torch tensors or ints). Pitches default to the width and strides to a
        dense frame; all in elements (the normals: stride in floats, pitch in pixels). Enqueued on the handle's stream;
        check() synchronises and reports a non-finite pose."""
        ds, dp = self._layout(width, height, depth_stride, depth_pitch, 1)
        ms, mp = self._layout(width, height, model_depth_stride, model_depth_pitch, 1)
        ns, np_ = self._layout(width, height, normal_stride, normal_pitch, 3)
        check(self._L.aria_icp_track_batch_device(self._h, _ptr(d_depth), ds, dp, _ptr(d_model_depth), ms, mp, _ptr(d_model_normal), ns,
                                                  np_, _ptr(d_model_extrinsics), _ptr(d_guess), _ptr(d_mask), n_frames, width, height,
                                                  _ptr(d_extrinsics_out), _ptr(d_results)), "aria_icp_track_batch_device")

    def debug_system(self, d_depth, d_model_depth, d_model_normal, d_model_extrinsics, d_trel, n_frames, width, height, stride,
                     d_system, depth_stride=None, depth_pitch=None, model_depth_stride=None, model_depth_pitch=None,
                     normal_stride=None, normal_pitch=None):
        """aria_icp_debug_system_device: the 29 int64 of one accumulation per frame at the given Trel on the level pixels of
        `stride`, into d_system [n_frames, 29]; no solve."""
        ds, dp = self._layout(width, height, depth_stride, depth_pitch, 1)
        ms, mp = self._layout(width, height, model_depth_stride, model_depth_pitch, 1)
        ns, np_ = self._layout(width, height, normal_stride, normal_pitch, 3)
        check(self._L.aria_icp_debug_system_device(self._h, _ptr(d_depth), ds, dp, _ptr(d_model_depth), ms, mp, _ptr(d_model_normal), ns,
                                                   np_, _ptr(d_model_extrinsics), _ptr(d_trel), n_frames, width, height, stride,
                                                   _ptr(d_system)), "aria_icp_debug_system_device")

    def track(self, depth, model_depth, model_normal, model_extrinsics, guess=None):
        """One frame from host arrays; blocks. Returns icp_ref.Track(T [12] doubles, result). guess defaults to the model's
        pose. A non-finite pose raises AriaError (ARIA_E_INVALID)."""
        D = np.ascontiguousarray(depth, np.float32)
        M = np.ascontiguousarray(model_depth, np.float32)
        N = np.ascontiguousarray(model_normal, np.float32)
        if D.ndim != 2 or M.shape != D.shape or N.shape != D.shape + (3,):
            raise ValueError("depth and model_depth are [H, W], model_normal is [H, W, 3]")
        Tm = np.ascontiguousarray(np.asarray(model_extrinsics, np.float64).reshape(-1))
        T0 = Tm if guess is None else np.ascontiguousarray(np.asarray(guess, np.float64).reshape(-1))
        if Tm.size != 12 or T0.size != 12:
            raise ValueError("poses are 12 doubles [R|t], row-major")
        T, rec = np.zeros(12), np.zeros(1, ICP_RESULT_DTYPE)
        check(self._L.aria_icp_track(self._h, D.ctypes.data, M.ctypes.data, N.ctypes.data, Tm.ctypes.data, T0.ctypes.data, D.shape[1],
                                     D.shape[0], T.ctypes.data, rec.ctypes.data), "aria_icp_track")
        return icp_ref.Track(T, rec[0])

    def algorithmic_bytes(self, width, height, n_frames):
        import ctypes as C
        return self._L.aria_icp_algorithmic_bytes(C.byref(self.config), width, height, n_frames)


__all__ = ["HipDenseTracker", "ICP_RESULT_DTYPE", "ICP_TERMS"]
