"""Obstacle alerts on the device (include/aria_orb_hip.h, "obstacle alerts"): an exact order statistic of the valid depths
inside three image zones and every detection box of a frame, a priority from class and distance, and per-key cooldowns
that persist along a track. aria_slam_amd.alert_ref is the definition and the device equals it bit for bit.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on another stream (torch's
default stream, another handle's) must be synchronised before a *_device call, or the handle must be created on that
stream. The defaults for band, percentiles and zone_alert_m are assumptions nobody has tuned on a recording."""
import ctypes as C

import numpy as np

from . import _lib, alert_ref
from ._handle import StageHandle
from ._lib import ALERT_EVENT_DTYPE, ALERT_MEAS_DTYPE, ALERT_SOURCES, ALERT_STATE_DTYPE, DETECTION_DTYPE, check
from .frontend import _ptr

_FIELDS = ("width", "height", "zone_top", "zone_bottom", "max_dets", "min_valid", "min_depth", "max_depth", "zone_alert_m",
           "default_depth", "crit_m", "high_m", "medium_m", "beep_m", "obstacle_dangerous", "max_events_per_frame")


class HipObstacleAlerter(StageHandle):
    """Binding of aria_alert_t. zone_pct / det_pct = (num, den); dangerous = up to 32 class ids; cooldown_ns = 4 values by
    priority LOW..CRITICAL."""

    _prefix, _config = "alert", _lib.AlertConfig

    def __init__(self, width=None, height=None, zone_top=None, zone_bottom=None, max_dets=None, min_valid=None, min_depth=None,
                 max_depth=None, zone_pct=None, det_pct=None, zone_alert_m=None, default_depth=None, crit_m=None, high_m=None,
                 medium_m=None, beep_m=None, obstacle_dangerous=None, dangerous=None, max_events_per_frame=None, cooldown_ns=None,
                 stream=None, device=0):
        cfg = self._default_config(device, stream)
        given = dict(width=width, height=height, zone_top=zone_top, zone_bottom=zone_bottom, max_dets=max_dets, min_valid=min_valid,
                     min_depth=min_depth, max_depth=max_depth, zone_alert_m=zone_alert_m, default_depth=default_depth, crit_m=crit_m,
                     high_m=high_m, medium_m=medium_m, beep_m=beep_m, obstacle_dangerous=obstacle_dangerous,
                     max_events_per_frame=max_events_per_frame)
        for name in _FIELDS:
            if given[name] is not None:
                setattr(cfg, name, given[name])
        if height is not None and zone_bottom is None:
            cfg.zone_bottom = cfg.height                                  # the band of another size: its lower three quarters
            if zone_top is None:
                cfg.zone_top = cfg.height // 4
        if zone_pct is not None:
            cfg.zone_pct_num, cfg.zone_pct_den = zone_pct
        if det_pct is not None:
            cfg.det_pct_num, cfg.det_pct_den = det_pct
        if dangerous is not None:
            ids = [int(v) for v in dangerous]
            if len(ids) > 32:
                raise ValueError("at most 32 dangerous class ids")
            cfg.n_dangerous = len(ids)
            for i in range(32):
                cfg.dangerous[i] = ids[i] if i < len(ids) else 0
        if cooldown_ns is not None:
            for i, v in enumerate(cooldown_ns):
                cfg.cooldown_ns[i] = int(v)
        self._create(cfg)

    @classmethod
    def from_ref_config(cls, c, **kw):
        """A handle of an alert_ref.Config."""
        d = {name: getattr(c, name) for name in _FIELDS}
        d.update(zone_pct=c.zone_pct, det_pct=c.det_pct, dangerous=c.dangerous, cooldown_ns=c.cooldown_ns)
        d.update(kw)
        return cls(**d)

    @property
    def ref_config(self):
        """The configuration as alert_ref.Config."""
        c = self.config
        d = {name: getattr(c, name) for name in _FIELDS}
        return alert_ref.config(zone_pct=(c.zone_pct_num, c.zone_pct_den), det_pct=(c.det_pct_num, c.det_pct_den),
                                dangerous=tuple(c.dangerous[:c.n_dangerous]), cooldown_ns=tuple(c.cooldown_ns), **d)

    @staticmethod
    def zone_bounds(width):
        """(first CENTER column, first RIGHT column) of rule 1 (aria_alert_zone_bounds, host only)."""
        out = (C.c_int * 2)()
        check(_lib.load_library().aria_alert_zone_bounds(width, out), "aria_alert_zone_bounds")
        return out[0], out[1]

    @staticmethod
    def new_state(n=1):
        """n cleared aria_alert_state records (all zero bytes)."""
        return np.zeros(n, ALERT_STATE_DTYPE)

    def dets_seen(self):
        """The largest detection count above max_dets met before the last check / status, 0 when none."""
        return self._L.aria_alert_dets_seen(self._h)

    def measure_batch_device(self, d_depth, depth_stride, depth_pitch, n_frames, d_meas, d_dets=None, d_ndets=None, det_cap=0):
        """aria_alert_measure_batch_device; enqueued."""
        check(self._L.aria_alert_measure_batch_device(self._h, _ptr(d_depth), depth_stride, depth_pitch, n_frames, _opt(d_dets),
                                                      _opt(d_ndets), det_cap, _ptr(d_meas)), "aria_alert_measure_batch_device")

    def arbitrate_batch_device(self, d_track_offset, n_tracks, d_timestamps, n_frames, d_meas, d_states, d_events, event_cap, d_nevents,
                               d_dets=None, d_ndets=None, det_cap=0):
        """aria_alert_arbitrate_batch_device; enqueued."""
        check(self._L.aria_alert_arbitrate_batch_device(self._h, _ptr(d_track_offset), n_tracks, _ptr(d_timestamps), n_frames, _ptr(d_meas),
                                                        _opt(d_dets), _opt(d_ndets), det_cap, _ptr(d_states), _opt(d_events), event_cap,
                                                        _ptr(d_nevents)), "aria_alert_arbitrate_batch_device")

    def run_batch_device(self, d_depth, depth_stride, depth_pitch, n_frames, d_track_offset, n_tracks, d_timestamps, d_states, d_events,
                         event_cap, d_nevents, d_dets=None, d_ndets=None, det_cap=0):
        """aria_alert_run_batch_device; enqueued."""
        check(self._L.aria_alert_run_batch_device(self._h, _ptr(d_depth), depth_stride, depth_pitch, n_frames, _opt(d_dets), _opt(d_ndets),
                                                  det_cap, _ptr(d_track_offset), n_tracks, _ptr(d_timestamps), _ptr(d_states), _opt(d_events),
                                                  event_cap, _ptr(d_nevents)), "aria_alert_run_batch_device")

    def _host_frames(self, depth, dets, ndets):
        depth = np.ascontiguousarray(depth, np.float32)
        if depth.ndim == 2:
            depth = depth[None]
        if depth.ndim != 3 or depth.shape[1] != self.config.height or depth.shape[2] < self.config.width:
            raise ValueError("depth is fp32 [n_frames, height, pitch >= width]")
        if (dets is None) != (ndets is None):
            raise ValueError("dets and ndets come together")
        det_cap = 0
        if dets is not None:
            dets = np.ascontiguousarray(dets, DETECTION_DTYPE).reshape(depth.shape[0], -1)
            ndets = np.ascontiguousarray(ndets, np.int32).reshape(depth.shape[0])
            det_cap = dets.shape[1]
        return depth, dets, ndets, det_cap

    def measure(self, depth, dets=None, ndets=None):
        """Rules 1-2 from host arrays; blocks. depth [F, H, pitch >= W]; dets [F, det_cap] DETECTION_DTYPE and ndets [F] or None.
        Returns (meas [F, 64], status): the status is not raised."""
        depth, dets, ndets, det_cap = self._host_frames(depth, dets, ndets)
        n = depth.shape[0]
        meas = np.zeros((n, ALERT_SOURCES), ALERT_MEAS_DTYPE)
        rc = self._L.aria_alert_measure(self._h, depth.ctypes.data, depth.shape[1] * depth.shape[2], depth.shape[2], n, _host(dets),
                                        _host(ndets), det_cap, meas.ctypes.data)
        return meas, rc

    def run(self, depth, timestamps, states, event_cap, track_offset=None, dets=None, ndets=None, events=None):
        """Rules 1-6 from host arrays; blocks. One track over all frames unless track_offset is given. states
        (ALERT_STATE_DTYPE, one per track) are advanced in place. Returns (events [n_tracks, event_cap], nevents [n_tracks],
        status): event slots beyond a track's events keep the bytes of `events` (zero without one)."""
        depth, dets, ndets, det_cap = self._host_frames(depth, dets, ndets)
        n = depth.shape[0]
        ts = np.ascontiguousarray(timestamps, np.int64).reshape(n)
        off = np.ascontiguousarray([0, n] if track_offset is None else track_offset, np.int32)
        n_tracks = len(off) - 1
        if states.dtype != ALERT_STATE_DTYPE or len(states) != n_tracks or not states.flags["C_CONTIGUOUS"]:
            raise ValueError("states: one contiguous ALERT_STATE_DTYPE record per track")
        ev = np.zeros((n_tracks, event_cap), ALERT_EVENT_DTYPE) if events is None else np.ascontiguousarray(events, ALERT_EVENT_DTYPE)
        nev = np.zeros(n_tracks, np.int32)
        rc = self._L.aria_alert_run(self._h, depth.ctypes.data, depth.shape[1] * depth.shape[2], depth.shape[2], n, _host(dets), _host(ndets),
                                    det_cap, off.ctypes.data, n_tracks, ts.ctypes.data, states.ctypes.data,
                                    ev.ctypes.data if ev.size else None, event_cap, nev.ctypes.data)
        return ev, nev, rc

    def arbitrate(self, track_offset, timestamps, meas, states, event_cap, dets=None, ndets=None, events=None):
        """Rules 3-6 from host arrays; blocks. As run(), from measurements [F, 64]."""
        meas = np.ascontiguousarray(meas, ALERT_MEAS_DTYPE).reshape(-1, ALERT_SOURCES)
        n = meas.shape[0]
        det_cap = 0
        if dets is not None:
            dets = np.ascontiguousarray(dets, DETECTION_DTYPE).reshape(n, -1)
            ndets = np.ascontiguousarray(ndets, np.int32).reshape(n)
            det_cap = dets.shape[1]
        ts = np.ascontiguousarray(timestamps, np.int64).reshape(n)
        off = np.ascontiguousarray(track_offset, np.int32)
        n_tracks = len(off) - 1
        if states.dtype != ALERT_STATE_DTYPE or len(states) != n_tracks or not states.flags["C_CONTIGUOUS"]:
            raise ValueError("states: one contiguous ALERT_STATE_DTYPE record per track")
        ev = np.zeros((n_tracks, event_cap), ALERT_EVENT_DTYPE) if events is None else np.ascontiguousarray(events, ALERT_EVENT_DTYPE)
        nev = np.zeros(n_tracks, np.int32)
        rc = self._L.aria_alert_arbitrate(self._h, off.ctypes.data, n_tracks, ts.ctypes.data if n else None, n,
                                          meas.ctypes.data if n else None, _host(dets), _host(ndets), det_cap, states.ctypes.data,
                                          ev.ctypes.data if ev.size else None, event_cap, nev.ctypes.data)
        return ev, nev, rc


def _opt(x):
    return None if x is None else _ptr(x)


def _host(a):
    return None if a is None else a.ctypes.data


def algorithmic_bytes(width, zone_top, zone_bottom, n_frames):
    return _lib.load_library().aria_alert_algorithmic_bytes(width, zone_top, zone_bottom, n_frames)
