"""Local bundle adjustment on the device (include/aria_orb_hip.h, "local bundle adjustment"): the poses and points of sliding
windows refined together, batched over windows. aria_slam_amd.ba_ref restates the stage in NumPy and is its definition; a
window here is the dict ba_ref.make_window builds (poses (P, 12), pose_fixed, points (N, 3), point_fixed, obs, K).

As with the other stage handles, the handle's own stream is non-blocking: device buffers filled on torch's default stream
must be synchronised before optimize_batch_device, or the adjuster must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import BA_OBS_DTYPE, BA_RESULT_DTYPE, check
from .ba_ref import EUROC_K, HUBER_DEFAULT, MIN_DEPTH_DEFAULT
from .frontend import _ptr


def _result_dict(rec):
    r = {k: (float(rec[k]) if BA_RESULT_DTYPE[k].kind == "f" else int(rec[k])) for k in BA_RESULT_DTYPE.names if k != "reserved"}
    r["lambda_"] = r.pop("lambda")
    r["record"] = rec.tobytes()          # the raw aria_ba_result (56 bytes)
    return r


def _arrays(win):
    return (np.ascontiguousarray(win["poses"], np.float64).reshape(-1, 12).copy(),
            np.ascontiguousarray(win["pose_fixed"], np.uint8).reshape(-1),
            np.ascontiguousarray(win["points"], np.float64).reshape(-1, 3).copy(),
            np.ascontiguousarray(win["point_fixed"], np.uint8).reshape(-1),
            np.ascontiguousarray(win["obs"], BA_OBS_DTYPE).reshape(-1))


def _p(a):
    return a.ctypes.data if a.size else None


class HipBundleAdjuster(StageHandle):
    """Binding of aria_ba_t. The intrinsics, the Huber width and min_depth belong to the handle."""

    _prefix, _config = "ba", _lib.BaConfig

    def __init__(self, K=EUROC_K, huber_px=HUBER_DEFAULT, min_depth=MIN_DEPTH_DEFAULT, max_iterations=10, max_windows=256,
                 stream=None, device=0):
        cfg = self._default_config(device, stream)
        cfg.fx, cfg.fy, cfg.cx, cfg.cy = K
        cfg.huber_px, cfg.min_depth = huber_px, min_depth
        cfg.max_iterations, cfg.max_windows = max_iterations, max_windows
        self._create(cfg)

    def optimize(self, win, iterations=0, raise_on_error=True):
        """One window, host arrays; blocks. Returns (poses (P, 12), points (N, 3), result dict with the aria_ba_result
        fields, `used` (the mask) and `status`). An invalid window raises unless raise_on_error is False."""
        poses, pf, pts, xf, obs = _arrays(win)
        res = np.zeros(1, BA_RESULT_DTYPE)
        used = np.zeros(max(len(obs), 1), np.uint8)
        rc = self._L.aria_ba_optimize(self._h, _p(poses), _p(pf), len(poses), _p(pts), _p(xf), len(pts), _p(obs), len(obs),
                                      iterations, res.ctypes.data, used.ctypes.data)
        if rc != 0 and (raise_on_error or rc != -1):
            check(rc, "aria_ba_optimize")
        out = _result_dict(res[0])
        out.update(used=used[:len(obs)], status=rc)
        return poses, pts, out

    def optimize_batch(self, windows, iterations=0, raise_on_error=True, pose_cap=None, point_cap=None, obs_cap=None):
        """Host windows through one aria_ba_optimize_batch_device call. Returns ([poses], [points], [result dict with
        `used`], status of aria_ba_check); raises on a deferred error unless told not to. A window's counts may be
        overridden by the keys n_poses / n_points / n_obs (to hand the device counts its records do not have)."""
        import torch

        B = len(windows)
        if B == 0:
            return [], [], [], 0
        arr = [_arrays(w) for w in windows]
        Pc = pose_cap or max(max(len(a[0]) for a in arr), 1)
        Nc = point_cap or max(max(len(a[2]) for a in arr), 1)
        Oc = obs_cap or max(max(len(a[4]) for a in arr), 1)
        poses, pf = np.zeros((B, Pc, 12)), np.zeros((B, Pc), np.uint8)
        pts, xf = np.zeros((B, Nc, 3)), np.zeros((B, Nc), np.uint8)
        obs = np.zeros((B, Oc), BA_OBS_DTYPE)
        counts = np.zeros((3, B), np.int32)
        for b, (a, w) in enumerate(zip(arr, windows)):
            poses[b, :len(a[0])], pf[b, :len(a[1])], pts[b, :len(a[2])], xf[b, :len(a[3])], obs[b, :len(a[4])] = a
            counts[:, b] = (w.get("n_poses", len(a[0])), w.get("n_points", len(a[2])), w.get("n_obs", len(a[4])))
        dev = torch.device("cuda", self.config.device)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
        dp, dpf, dx, dxf, do, dn = d(poses), d(pf), d(pts), d(xf), d(obs), d(counts)
        dres = torch.zeros(B * BA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        dused = torch.full((B * Oc,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)          # the handle's own stream is not ordered against torch's default stream
        self.optimize_batch_device(dp, dpf, dx, dxf, do, dn.data_ptr(), dn.data_ptr() + 4 * B, dn.data_ptr() + 8 * B, B, Pc,
                                   Nc, Oc, iterations, dres, dused)
        status = self.status()
        if status != 0 and raise_on_error:
            check(status, "aria_ba_check")
        op = np.frombuffer(dp.cpu().numpy().tobytes(), np.float64).reshape(B, Pc, 12)
        ox = np.frombuffer(dx.cpu().numpy().tobytes(), np.float64).reshape(B, Nc, 3)
        res = np.frombuffer(dres.cpu().numpy().tobytes(), BA_RESULT_DTYPE)
        used = dused.cpu().numpy().reshape(B, Oc)
        out = []
        for b, a in enumerate(arr):
            r = _result_dict(res[b])
            r["used"] = used[b, :len(a[4])].copy()
            r["used_tail"] = used[b, len(a[4]):].copy()
            out.append(r)
        return ([op[b, :len(a[0])].copy() for b, a in enumerate(arr)], [ox[b, :len(a[2])].copy() for b, a in enumerate(arr)],
                out, status)

    def optimize_batch_device(self, d_poses, d_pose_fixed, d_points, d_point_fixed, d_obs, d_n_poses, d_n_points, d_n_obs,
                              n_windows, pose_cap, point_cap, obs_cap, iterations, d_results, d_used=None):
        """aria_ba_optimize_batch_device: device pointers (torch tensors or ints). Poses and points are updated in place;
        d_results: n_windows * 56 bytes (BA_RESULT_DTYPE); d_used (optional): n_windows * obs_cap bytes. Enqueued on the
        handle's stream; check() synchronises."""
        check(self._L.aria_ba_optimize_batch_device(self._h, _ptr(d_poses), _ptr(d_pose_fixed), _ptr(d_points),
                                                    _ptr(d_point_fixed), _ptr(d_obs), _ptr(d_n_poses), _ptr(d_n_points),
                                                    _ptr(d_n_obs), n_windows, pose_cap, point_cap, obs_cap, iterations,
                                                    _ptr(d_results), _ptr(d_used) if d_used is not None else None),
              "aria_ba_optimize_batch_device")

    def window_from_chain_device(self, mapper, d_pair_first, d_n_pairs, n_windows, pair_base, n_chain_pairs, d_kp1, d_n1, d_kp2,
                                 d_n2, kp_stride, d_matches, d_nmatches, match_cap, point_cap, obs_cap, d_points, d_obs,
                                 d_point_src, d_n_points, d_n_obs, query_is_first=True):
        """aria_ba_window_from_chain_device: the windows' points and observations from the points of `mapper` (a HipMapper)
        and the chain's keypoints and matches, all device pointers. Enqueued on the handle's stream, which must be ordered
        after the work that filled the map; check() synchronises and reports a refused window."""
        check(self._L.aria_ba_window_from_chain_device(
            self._h, mapper._h, _ptr(d_pair_first), _ptr(d_n_pairs), n_windows, pair_base, n_chain_pairs, _ptr(d_kp1), _ptr(d_n1),
            _ptr(d_kp2), _ptr(d_n2), kp_stride, _ptr(d_matches), _ptr(d_nmatches), match_cap, 1 if query_is_first else 0,
            point_cap, obs_cap, _ptr(d_points), _ptr(d_obs), _ptr(d_point_src), _ptr(d_n_points), _ptr(d_n_obs)),
            "aria_ba_window_from_chain_device")

    def debug_linearize(self, win, lam):
        """dict(chi2, n_obs_used, S (6F, 6F), g (6F,), V (N, 3, 3), bp (N, 3)) of one window at its state, damped with lam."""
        poses, pf, pts, xf, obs = _arrays(win)
        F = int((pf == 0).sum())
        chi2, n_used = C.c_double(), C.c_int()
        S, g = np.zeros((max(6 * F, 1), max(6 * F, 1))), np.zeros(max(6 * F, 1))
        V, bp = np.zeros((max(len(pts), 1), 3, 3)), np.zeros((max(len(pts), 1), 3))
        check(self._L.aria_ba_debug_linearize(self._h, _p(poses), _p(pf), len(poses), _p(pts), _p(xf), len(pts), _p(obs),
                                              len(obs), float(lam), C.byref(chi2), C.byref(n_used), S.ctypes.data, g.ctypes.data,
                                              V.ctypes.data, bp.ctypes.data), "aria_ba_debug_linearize")
        return dict(chi2=chi2.value, n_obs_used=n_used.value, S=S.reshape(-1)[:36 * F * F].reshape(6 * F, 6 * F), g=g[:6 * F],
                    V=V[:len(pts)], bp=bp[:len(pts)])
