"""Trajectory evaluation on the device (include/aria_orb_hip.h, "trajectory evaluation"): the reference's ground-truth lookup
(EuRoCReader::getGroundTruth, src/legacy/EuRoCReader.cpp:311-346), its ATE / RPE (src/euroc_eval.cpp:28-61) and the
Umeyama-aligned figures, batched over query timestamps and over trajectories. aria_slam_amd.eval_ref restates all of it in
NumPy and is the definition.

HipTrajectoryEvaluator.sample_ground_truth and evaluate_batch take host arrays and block; evaluate_batch_device and
sample_ground_truth_device take device pointers (torch tensors or ints), so the poses that optimize_batch_device or
run_batch_device left in HBM are scored where they lie and only the result records come back.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_device call, or the object must be created on the caller's stream."""

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import (EVAL_EST_FUSE_STATE, EVAL_EST_POSE12, EVAL_EST_XYZ, EVAL_RESULT_DTYPE, EVAL_TRUTH_DTYPE, FUSE_STATE_DTYPE,
                   check)
from .frontend import _ptr

ALIGN_MODES = {"none": _lib.EVAL_ALIGN_NONE, "se3": _lib.EVAL_ALIGN_SE3, "sim3": _lib.EVAL_ALIGN_SIM3}


def load_ground_truth_csv(path):
    """EuRoCReader::loadGroundTruth (src/legacy/EuRoCReader.cpp:157-216) on one data.csv: the first line is skipped, so are
    empty lines and lines starting with '#', rows of fewer than 17 fields are dropped, the first 17 fields of the others are
    read (timestamp in nanoseconds -> seconds), and the rows are sorted by timestamp. The sort is stable, ours by definition
    (std::sort promises nothing for equal keys). Returns EVAL_TRUTH_DTYPE records; a file without usable rows gives none."""
    rows = []
    with open(path) as f:
        f.readline()
        for line in f:
            line = line.rstrip("\r\n")
            if not line or line[0] == "#":
                continue
            tok = line.split(",")
            if len(tok) < 17:
                continue
            rows.append([float(tok[0]) * 1e-9] + [float(x) for x in tok[1:17]])
    a = np.array(rows, np.float64).reshape(-1, 17)
    a = a[np.argsort(a[:, 0], kind="stable")]
    return pack_truth(a)


def pack_truth(rows):
    """(M, 17) rows [t, p, q (w, x, y, z), v, bg, ba] (or EVAL_TRUTH_DTYPE records) -> contiguous EVAL_TRUTH_DTYPE records."""
    if isinstance(rows, np.ndarray) and rows.dtype == EVAL_TRUTH_DTYPE:
        return np.ascontiguousarray(rows).reshape(-1)
    a = np.ascontiguousarray(np.asarray(rows, np.float64).reshape(-1, 17))
    return a.view(EVAL_TRUTH_DTYPE).reshape(-1).copy()


def truth_from_positions(pos):
    """EVAL_TRUTH_DTYPE records that carry the positions (n, 3) and an identity orientation: truth for evaluate_batch that
    did not come from the sampler."""
    p = np.asarray(pos, np.float64).reshape(-1, 3)
    rec = np.zeros(len(p), EVAL_TRUTH_DTYPE)
    rec["p"] = p
    rec["q"][:, 0] = 1.0
    return rec


def _pack_est(est):
    """One trajectory's estimate -> (kind, contiguous array): FUSE_STATE_DTYPE records, (n, 4, 4) / (n, 3, 4) / (n, 12) pose
    rows, or (n, 3) positions."""
    if isinstance(est, np.ndarray) and est.dtype == FUSE_STATE_DTYPE:
        return EVAL_EST_FUSE_STATE, np.ascontiguousarray(est).reshape(-1)
    a = np.asarray(est, np.float64)
    if a.ndim == 3 and a.shape[1:] in ((4, 4), (3, 4)):
        return EVAL_EST_POSE12, np.ascontiguousarray(a[:, :3, :].reshape(-1, 12))
    if a.ndim == 2 and a.shape[1] == 12:
        return EVAL_EST_POSE12, np.ascontiguousarray(a)
    return EVAL_EST_XYZ, np.ascontiguousarray(a.reshape(-1, 3))


def _align(mode, default):
    if mode is None:
        return default
    return ALIGN_MODES[mode] if isinstance(mode, str) else int(mode)


class HipTrajectoryEvaluator(StageHandle):
    """Binding of aria_eval_t."""

    _prefix, _config = "eval", _lib.EvalConfig

    def __init__(self, stream=None, device=0, align="sim3", rpe_delta=10):
        cfg = self._default_config(device, stream)
        cfg.align_mode = _align(align, cfg.align_mode)
        cfg.rpe_delta = rpe_delta
        self._create(cfg)
        self.last_status = 0

    # ---- ground truth
    def sample_ground_truth(self, gt, timestamps, raise_on_error=True):
        """Host arrays; blocks. gt: (M, 17) rows or EVAL_TRUTH_DTYPE records; returns (EVAL_TRUTH_DTYPE records, valid (n,))."""
        g = pack_truth(gt)
        ts = np.ascontiguousarray(timestamps, np.float64).reshape(-1)
        out, valid = np.zeros(len(ts), EVAL_TRUTH_DTYPE), np.zeros(len(ts), np.int32)
        self.last_status = self._L.aria_eval_sample_truth(self._h, g.ctypes.data if len(g) else None, len(g),
                                                          ts.ctypes.data if len(ts) else None, len(ts),
                                                          out.ctypes.data if len(ts) else None, valid.ctypes.data if len(ts) else None)
        if self.last_status != 0 and (raise_on_error or self.last_status != -1):
            check(self.last_status, "aria_eval_sample_truth")
        return out, valid

    def sample_ground_truth_device(self, d_gt, n_gt, d_timestamps, n, d_out, d_valid=None):
        """aria_eval_sample_truth_device: device pointers. Enqueued on the handle's stream; check() synchronises."""
        check(self._L.aria_eval_sample_truth_device(self._h, _ptr(d_gt), n_gt, _ptr(d_timestamps), n, _ptr(d_out), _ptr(d_valid)),
              "aria_eval_sample_truth_device")

    # ---- metrics
    def evaluate_batch(self, estimates, truth, shared_truth=False, masks=None, align=None, rpe_delta=None, pose_errors=False,
                       raise_on_error=True):
        """Host arrays through one aria_eval_batch call; blocks. estimates: a list of trajectories, all of one kind (see
        _pack_est). truth: a list of per-trajectory truths (EVAL_TRUTH_DTYPE records or (n, 3) positions), or with
        shared_truth one such truth for all. masks: None or a list of per-trajectory byte masks (None entries = all used).
        Returns EVAL_RESULT_DTYPE records, or (records, [per-pose aligned errors]) with pose_errors. An invalid trajectory
        (valid = 0) raises unless told not to; self.last_status keeps the status."""
        packed = [_pack_est(e) for e in estimates]
        kinds = {k for k, _ in packed}
        assert len(kinds) <= 1, "one estimate kind per call"
        kind = kinds.pop() if kinds else EVAL_EST_XYZ
        B = len(packed)
        off = np.concatenate([[0], np.cumsum([len(a) for _, a in packed])]).astype(np.int32)
        NP = int(off[-1])
        tr = lambda t: t if isinstance(t, np.ndarray) and t.dtype == EVAL_TRUTH_DTYPE else truth_from_positions(t)
        if shared_truth:
            allt = np.ascontiguousarray(tr(truth))
        else:
            assert len(truth) == B
            allt = np.concatenate([tr(t) for t in truth] + [np.zeros(0, EVAL_TRUTH_DTYPE)])
        if kind == EVAL_EST_FUSE_STATE:
            alle = np.concatenate([a for _, a in packed] + [np.zeros(0, FUSE_STATE_DTYPE)])
        else:
            alle = np.concatenate([a for _, a in packed] + [np.zeros((0, 12 if kind == EVAL_EST_POSE12 else 3))])
        allm = None
        if masks is not None:
            allm = np.concatenate([np.ones(len(a), np.uint8) if m is None else (np.asarray(m).reshape(-1) != 0).astype(np.uint8)
                                   for (_, a), m in zip(packed, masks)] + [np.zeros(0, np.uint8)])
            assert len(allm) == NP
        res = np.zeros(B, EVAL_RESULT_DTYPE)
        err = np.zeros(max(NP, 1), np.float64) if pose_errors else None
        if B:
            self.last_status = self._L.aria_eval_batch(
                self._h, alle.ctypes.data if NP else None, kind, off.ctypes.data, NP, B, allt.ctypes.data if len(allt) else None,
                len(allt), int(bool(shared_truth)), None if allm is None or NP == 0 else allm.ctypes.data,
                _align(align, self.config.align_mode), self.config.rpe_delta if rpe_delta is None else int(rpe_delta),
                None if err is None else err.ctypes.data, res.ctypes.data)
            if self.last_status != 0 and (raise_on_error or self.last_status != -1):
                check(self.last_status, "aria_eval_batch")
        if pose_errors:
            return res, [err[off[k]:off[k + 1]].copy() for k in range(B)]
        return res

    def evaluate_batch_device(self, d_est, est_kind, d_offset, n_poses_total, n_traj, d_truth, n_truth, d_results, truth_shared=False,
                              d_mask=None, align=None, rpe_delta=None, d_pose_err=None):
        """aria_eval_batch_device: device pointers (torch tensors or ints). d_est / d_offset may be the d_poses /
        d_vertex_offset of optimize_batch_device (est_kind EVAL_EST_POSE12) or the d_states / d_frame_offset of
        run_batch_device (EVAL_EST_FUSE_STATE). d_results: n_traj * 200 bytes (EVAL_RESULT_DTYPE). Enqueued on the handle's
        stream; check() synchronises."""
        check(self._L.aria_eval_batch_device(self._h, _ptr(d_est), est_kind, _ptr(d_offset), n_poses_total, n_traj, _ptr(d_truth),
                                             n_truth, int(bool(truth_shared)), _ptr(d_mask), _align(align, self.config.align_mode),
                                             self.config.rpe_delta if rpe_delta is None else int(rpe_delta), _ptr(d_pose_err),
                                             _ptr(d_results)), "aria_eval_batch_device")
