"""Visual-inertial fusion on the device (include/aria_orb_hip.h, "visual-inertial fusion"): the reference's SensorFusion EKF
(include/legacy/IMU.hpp:53-118, src/legacy/IMU.cpp:102-305) batched over tracks, and its IMUPreintegrator (IMU.cpp:28-100)
batched over image intervals. aria_slam_amd.fusion_ref restates both in NumPy and is their definition.

HipSensorFusion carries the reference class's surface (add_imu, add_visual_pose, the getters): events are queued on the host
and flushed through aria_fuse_run when a getter is called, the filter record travelling with them. run_batch takes host
tracks, run_batch_device and visual_from_pose_device device pointers. HipImuPreintegrator does the same for intervals.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_device call, or the object must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import (FUSE_FILTER_DTYPE, FUSE_STATE_DTYPE, FUSE_VISUAL_DTYPE, IMU_SAMPLE_DTYPE, PREINT_RESULT_DTYPE, check)
from .frontend import _ptr


def pack_imu(imu):
    """(N, 7) rows [t, accel, gyro] (or IMU_SAMPLE_DTYPE records) -> contiguous IMU_SAMPLE_DTYPE records."""
    if isinstance(imu, np.ndarray) and imu.dtype == IMU_SAMPLE_DTYPE:
        return np.ascontiguousarray(imu)
    a = np.ascontiguousarray(np.asarray(imu, np.float64).reshape(-1, 7))
    return a.view(IMU_SAMPLE_DTYPE).reshape(-1).copy()


def pack_visual(visual):
    """[(t, R 3x3, p 3, accept)] (or FUSE_VISUAL_DTYPE records) -> FUSE_VISUAL_DTYPE records."""
    if isinstance(visual, np.ndarray) and visual.dtype == FUSE_VISUAL_DTYPE:
        return np.ascontiguousarray(visual)
    rec = np.zeros(len(visual), FUSE_VISUAL_DTYPE)
    for k, (t, R, p, accept) in enumerate(visual):
        rec[k] = (t, np.asarray(R, np.float64).reshape(9), np.asarray(p, np.float64).reshape(3), int(bool(accept)), 0)
    return rec


def new_filter(n=1, gravity=None, **noise):
    """n aria_fuse_filter records as aria_fuse_filter_init leaves them; gravity / noise constants override the defaults."""
    L = _lib.load_library()
    cfg = _lib.FuseConfig()
    L.aria_fuse_default_config(C.byref(cfg))
    if gravity is not None:
        cfg.gravity[:] = [float(g) for g in gravity]
    for k, v in noise.items():
        if k not in ("accel_noise", "gyro_noise", "accel_bias_walk", "gyro_bias_walk", "pos_noise", "rot_noise"):
            raise TypeError("unknown noise constant %r" % k)
        setattr(cfg, k, float(v))
    one = np.zeros(1, FUSE_FILTER_DTYPE)
    check(L.aria_fuse_filter_init(one.ctypes.data, C.byref(cfg)), "aria_fuse_filter_init")
    return np.repeat(one, n)


def filter_from_ref(flt):
    """A fusion_ref.SensorFusion as one FUSE_FILTER_DTYPE record (rounded to fp64)."""
    rec = np.zeros(1, FUSE_FILTER_DTYPE)
    r = rec[0]
    r["p"], r["v"], r["q"] = flt.position, flt.velocity, flt.orientation
    r["ba"], r["bg"] = flt.accel_bias, flt.gyro_bias
    r["P"] = np.asarray(flt.P, np.float64).reshape(225)
    r["last_imu_time"], r["last_visual_time"] = float(flt.last_imu_time), float(flt.last_visual_time)
    r["gravity"] = flt.gravity
    for k, v in flt.noise.items():
        r[k] = float(v)
    r["initialized"] = int(flt.initialized)
    return rec


class _FuseHandle(StageHandle):
    _prefix, _config = "fuse", _lib.FuseConfig

    def __init__(self, stream=None, device=0):
        cfg = self._default_config(device, stream)
        self._create(cfg)


class HipSensorFusion(_FuseHandle):
    """Binding of aria_fuse_t behind the reference class's methods."""

    def __init__(self, stream=None, device=0, gravity=None, **noise):
        super().__init__(stream, device)
        self.filter = new_filter(1, gravity, **noise)
        self._imu, self._imu_end, self._visual = [], [], []
        self.last_states = np.zeros(0, FUSE_STATE_DTYPE)

    # ---- the reference class's surface: events are queued, a getter flushes them through one aria_fuse_run
    def add_imu(self, t, accel, gyro):
        self._imu.append((float(t),) + tuple(float(x) for x in accel) + tuple(float(x) for x in gyro))

    def add_visual_pose(self, t, R, p):
        self._imu_end.append(len(self._imu))
        self._visual.append((t, R, p, 1))

    def flush(self):
        if self._imu and (not self._imu_end or self._imu_end[-1] < len(self._imu)):
            # samples after the last visual pose: a frame without a measurement consumes them
            self._imu_end.append(len(self._imu))
            self._visual.append((self._imu[-1][0], np.eye(3), np.zeros(3), 0))
        if not self._visual:
            return
        self.last_states = self.run(np.array(self._imu, np.float64).reshape(-1, 7), self._imu_end, self._visual)
        self._imu, self._imu_end, self._visual = [], [], []

    def get_position(self):
        self.flush()
        return self.filter[0]["p"].copy()

    def get_velocity(self):
        self.flush()
        return self.filter[0]["v"].copy()

    def get_orientation(self):
        """(w, x, y, z)."""
        self.flush()
        return self.filter[0]["q"].copy()

    def get_bias(self):
        self.flush()
        return self.filter[0]["ba"].copy(), self.filter[0]["bg"].copy()

    def get_covariance(self):
        self.flush()
        return self.filter[0]["P"].reshape(15, 15).copy()

    def is_initialized(self):
        self.flush()
        return bool(self.filter[0]["initialized"])

    # ---- arrays
    def run(self, imu, imu_end, visual, filt=None):
        """One track through aria_fuse_run, host arrays; blocks. Updates self.filter (or `filt`, one FUSE_FILTER_DTYPE
        record, in place) and returns the per-frame FUSE_STATE_DTYPE records."""
        filt = self.filter if filt is None else filt
        assert filt.dtype == FUSE_FILTER_DTYPE and filt.flags["C_CONTIGUOUS"] and len(filt) == 1
        s, v = pack_imu(imu), pack_visual(visual)
        e = np.ascontiguousarray(imu_end, np.int32)
        assert len(e) == len(v)
        states = np.zeros(len(v), FUSE_STATE_DTYPE)
        check(self._L.aria_fuse_run(self._h, filt.ctypes.data, s.ctypes.data if len(s) else None, len(s),
                                    e.ctypes.data if len(e) else None, v.ctypes.data if len(v) else None, len(v),
                                    states.ctypes.data if len(v) else None), "aria_fuse_run")
        return states

    def run_batch(self, tracks, filters=None, raise_on_error=True):
        """tracks: [(imu (N, 7), imu_end (F,), visual)]. One aria_fuse_run_batch_device call over all of them. filters:
        FUSE_FILTER_DTYPE records, one per track (default: fresh ones). Returns (filters after, [states per track], status
        of aria_fuse_check); raises on a deferred error unless told not to."""
        import torch

        B = len(tracks)
        filters = new_filter(B) if filters is None else np.ascontiguousarray(filters).copy()
        if B == 0:
            return filters, [], 0
        assert filters.dtype == FUSE_FILTER_DTYPE and len(filters) == B
        imus = [pack_imu(t[0]) for t in tracks]
        ends = [np.asarray(t[1], np.int32).reshape(-1) for t in tracks]
        viss = [pack_visual(t[2]) for t in tracks]
        ioff = np.concatenate([[0], np.cumsum([len(x) for x in imus])]).astype(np.int32)
        foff = np.concatenate([[0], np.cumsum([len(x) for x in viss])]).astype(np.int32)
        allimu = np.concatenate(imus + [np.zeros(1, IMU_SAMPLE_DTYPE)])          # never empty
        allend = np.concatenate(ends + [np.zeros(1, np.int32)])
        allvis = np.concatenate(viss + [np.zeros(1, FUSE_VISUAL_DTYPE)])
        dev = torch.device("cuda", self.config.device)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
        dflt, dimu, dio, dend, dvis, dfo = d(filters), d(allimu), d(ioff), d(allend), d(allvis), d(foff)
        dst = torch.zeros((int(foff[-1]) + 1) * FUSE_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)          # the handle's own stream is not ordered against torch's default stream
        self.run_batch_device(dflt, dimu, dio, int(ioff[-1]), dend, dvis, dfo, int(foff[-1]), B, dst)
        status = self.status()
        if status != 0 and raise_on_error:
            check(status, "aria_fuse_check")
        out_f = np.frombuffer(dflt.cpu().numpy().tobytes(), FUSE_FILTER_DTYPE).copy()
        st = np.frombuffer(dst.cpu().numpy().tobytes(), FUSE_STATE_DTYPE)
        return out_f, [st[foff[k]:foff[k + 1]].copy() for k in range(B)], status

    def run_batch_device(self, d_filters, d_imu, d_imu_offset, n_imu_total, d_imu_end, d_visual, d_frame_offset, n_frames_total,
                         n_tracks, d_states):
        """aria_fuse_run_batch_device: device pointers (torch tensors or ints). Enqueued on the handle's stream; check()
        synchronises."""
        check(self._L.aria_fuse_run_batch_device(self._h, _ptr(d_filters), _ptr(d_imu), _ptr(d_imu_offset), n_imu_total,
                                                 _ptr(d_imu_end), _ptr(d_visual), _ptr(d_frame_offset), n_frames_total,
                                                 n_tracks, _ptr(d_states)), "aria_fuse_run_batch_device")

    def visual_from_pose_device(self, d_pose_results, d_timestamps, n, min_pose_inliers, d_visual):
        """aria_fuse_visual_from_pose_device: n aria_pose_result records and n doubles in HBM -> n aria_fuse_visual records."""
        check(self._L.aria_fuse_visual_from_pose_device(self._h, _ptr(d_pose_results), _ptr(d_timestamps), n, min_pose_inliers,
                                                        _ptr(d_visual)), "aria_fuse_visual_from_pose_device")


class HipImuPreintegrator(_FuseHandle):
    """IMUPreintegrator over many intervals of one sample array."""

    def preintegrate(self, imu, begin, end, bias=None, raise_on_error=True):
        """Host arrays; blocks. Returns PREINT_RESULT_DTYPE records, one per interval [begin[i], end[i]); an invalid interval
        (valid = 0, zeroed) raises unless told not to, self.last_status keeps aria_fuse_preintegrate's status."""
        s = pack_imu(imu)
        b, e = np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(end, np.int32)
        assert len(b) == len(e)
        out = np.zeros(len(b), PREINT_RESULT_DTYPE)
        bs = None if bias is None else np.ascontiguousarray(bias, np.float64).reshape(6)
        self.last_status = self._L.aria_fuse_preintegrate(self._h, s.ctypes.data if len(s) else None, len(s),
                                                          b.ctypes.data if len(b) else None, e.ctypes.data if len(b) else None,
                                                          len(b), None if bs is None else bs.ctypes.data,
                                                          out.ctypes.data if len(b) else None)
        if self.last_status != 0 and (raise_on_error or self.last_status != -1):
            check(self.last_status, "aria_fuse_preintegrate")
        return out

    def preintegrate_device(self, d_imu, n_imu, d_begin, d_end, n_intervals, d_bias, d_out):
        """aria_fuse_preintegrate_batch_device: device pointers. Enqueued on the handle's stream; check() synchronises."""
        check(self._L.aria_fuse_preintegrate_batch_device(self._h, _ptr(d_imu), n_imu, _ptr(d_begin), _ptr(d_end), n_intervals,
                                                          _ptr(d_bias), _ptr(d_out)), "aria_fuse_preintegrate_batch_device")
