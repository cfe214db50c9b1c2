"""NumPy restatement of frame-to-model tracking (include/aria_orb_hip.h, "frame-to-model tracking"): batched point-to-plane
ICP of a live fp32 depth map against the depth map and world-frame normals that the ray casting stage predicted from the
volume. The reference has no code for it (KinectFusion's tracking step), so this file IS the definition and the device equals
it bit for bit.

The per-pixel work (rule 3) is fp32 with one rounding per operation in the order the header writes it: np.float32 arrays and
scalars throughout. The normal equations (rule 4) are 29 int64 sums of fp64 products scaled by a power of two and rounded
half-even: integer addition is associative, so any reduction order gives these integers. The solve (rule 5) is scalar fp64 in
a stated order, written below with Python floats (IEEE doubles; + - * / and math.sqrt are correctly rounded)."""
import math
from collections import namedtuple

import numpy as np

from .tsdf_ref import EUROC_K

RESULT_DTYPE = np.dtype([("valid", "<i4"), ("iterations_run", "<i4"), ("n_corr", "<i4"), ("level", "<i4"), ("rms", "<f8"),
                         ("delta", "<f8")])                          # aria_icp_result, 32 bytes

MAX_LEVELS, MAX_STRIDE, MAX_ITERATIONS, MAX_PIXELS = 4, 16, 64, 1 << 24
MAX_DIST, MAX_REACH = 1.0, 128.0
NORMAL_MAX = 1.5                                                      # rule 3: (n.n) <= 1.5f
SCALE_A, SCALE_B, SCALE_R = 2.0 ** 24, 2.0 ** 30, 2.0 ** 36           # rule 4
N_TERMS = 29
# Rule 4's bound on one term before scaling: |q| <= reach (1 + 2^-22), |n| <= sqrt(1.5) (1 + 2^-22), |e| <= dist_max (1 + 2^-22).
J_MAX = MAX_REACH * math.sqrt(NORMAL_MAX) * (1 + 2.0 ** -20)          # a component of q x n; those of n are smaller
R_MAX = MAX_DIST * math.sqrt(NORMAL_MAX) * (1 + 2.0 ** -20)
TERM_MAX = (J_MAX * J_MAX * SCALE_A, J_MAX * R_MAX * SCALE_B, R_MAX * R_MAX * SCALE_R)

# min_pivot: the geometric mean of the least pivot / count over the valid cases of tests/icp_cases.py (1.42e-2) and the greatest
# pivot / count at which its `plane` case is lost (2.12e-9), both measured with this file (5.49e-6, rounded); tests/test_icp_host.py asserts that
# each lies 10x away.
DEFAULTS = dict(K=EUROC_K, min_depth=0.3, max_depth=10.0, dist_max=0.1, reach=64.0, min_corr=64, min_pivot=5e-6, eps=1e-6,
                strides=(4, 2, 1), iterations=(4, 5, 10))

Config = namedtuple("Config", "K min_depth max_depth dist_max reach min_corr min_pivot eps strides iterations")

f32 = np.float32


def config(**kw):
    """A Config from DEFAULTS and the overrides; raises ValueError where aria_icp_create returns ARIA_E_INVALID."""
    d = dict(DEFAULTS)
    d.update(kw)
    c = Config(K=tuple(float(v) for v in d["K"]), min_depth=f32(d["min_depth"]), max_depth=f32(d["max_depth"]),
               dist_max=f32(d["dist_max"]), reach=f32(d["reach"]), min_corr=int(d["min_corr"]), min_pivot=float(d["min_pivot"]),
               eps=float(d["eps"]), strides=tuple(int(v) for v in d["strides"]), iterations=tuple(int(v) for v in d["iterations"]))
    ok = len(c.K) == 4 and all(np.isfinite(v) for v in c.K) and c.K[0] != 0 and c.K[1] != 0
    ok = ok and np.isfinite(c.min_depth) and np.isfinite(c.max_depth) and c.min_depth > 0 and c.min_depth <= c.max_depth
    ok = ok and c.dist_max > 0 and c.dist_max <= f32(MAX_DIST) and c.reach > 0 and c.reach <= f32(MAX_REACH)
    ok = ok and 1 <= c.min_corr <= MAX_PIXELS and np.isfinite(c.min_pivot) and c.min_pivot >= 0 and np.isfinite(c.eps) and c.eps >= 0
    ok = ok and 1 <= len(c.strides) <= MAX_LEVELS and len(c.iterations) == len(c.strides)
    ok = ok and all(s in (1, 2, 4, 8, 16) for s in c.strides) and all(0 <= n <= MAX_ITERATIONS for n in c.iterations)
    ok = ok and sum(c.iterations) >= 1
    if not ok:
        raise ValueError("invalid tracking configuration")
    return c


def check_size(W, H):
    if W < 1 or H < 1 or W > 16384 or H > 16384 or W * H > MAX_PIXELS:
        raise ValueError("width x height outside 1..2^24 pixels")


# ---- rule 1: the state ------------------------------------------------------------------------------------------------------
def relative(Tm, T0):
    """Trel = Tm o T0^-1 as 12 Python floats [R|t] row-major: live camera to model camera."""
    Tm, T0 = [float(v) for v in Tm], [float(v) for v in T0]
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (Tm[4 * i] * T0[4 * j] + Tm[4 * i + 1] * T0[4 * j + 1]) + Tm[4 * i + 2] * T0[4 * j + 2]
    for i in range(3):
        out[4 * i + 3] = Tm[4 * i + 3] - ((out[4 * i] * T0[3] + out[4 * i + 1] * T0[7]) + out[4 * i + 2] * T0[11])
    return out


def model_rotation(Tm):
    """Rm as fp32, row-major: what rotates a model normal into the model camera frame."""
    e = np.asarray(Tm, np.float64).reshape(12).astype(f32)
    return [e[0], e[1], e[2], e[4], e[5], e[6], e[8], e[9], e[10]]


def output_pose(Trel, Tm):
    """Rule 6: T = Trel^-1 o Tm, 12 doubles."""
    Tm = [float(v) for v in Tm]
    out = np.zeros(12)
    d = [Tm[3] - Trel[3], Tm[7] - Trel[7], Tm[11] - Trel[11]]
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (Trel[i] * Tm[j] + Trel[4 + i] * Tm[4 + j]) + Trel[8 + i] * Tm[8 + j]
        out[4 * i + 3] = (Trel[i] * d[0] + Trel[4 + i] * d[1]) + Trel[8 + i] * d[2]
    return out


# ---- rules 3 and 4: one accumulation -----------------------------------------------------------------------------------------
def jacobians(cfg, D, M, N, Trel, Rm, stride):
    """Rule 3 for the level pixels of `stride`: (ok [n] bool, J [n, 6] fp32, r [n] fp32, um, vm), rows where ok is False zeroed.
    D: fp32 [H, W]; M: fp32 [H, W]; N: fp32 [H, W, 3]; Trel: 12 doubles; Rm: 9 fp32."""
    H, W = D.shape
    with np.errstate(all="ignore"):
        T = np.asarray(Trel, np.float64).astype(f32)
        fx, fy, cx, cy = (f32(v) for v in cfg.K)
        inv_fx, inv_fy = f32(1.0) / fx, f32(1.0) / fy
        uu, vv = np.meshgrid(np.arange(0, W, stride), np.arange(0, H, stride))
        uu, vv = uu.reshape(-1), vv.reshape(-1)
        d = np.asarray(D, f32)[vv, uu]
        ok = (d >= cfg.min_depth) & (d <= cfg.max_depth)
        p = [((uu.astype(f32) - cx) * inv_fx) * d, ((vv.astype(f32) - cy) * inv_fy) * d, d]
        q = [((T[4 * i] * p[0] + T[4 * i + 1] * p[1]) + T[4 * i + 2] * p[2]) + T[4 * i + 3] for i in range(3)]
        ok &= q[2] > f32(0)
        iz = f32(1.0) / q[2]
        um, vm = np.rint((fx * q[0]) * iz + cx), np.rint((fy * q[1]) * iz + cy)
        ok &= (um >= f32(0)) & (um <= f32(W - 1)) & (vm >= f32(0)) & (vm <= f32(H - 1))
        ui, vi = np.where(ok, um, f32(0)).astype(np.int64), np.where(ok, vm, f32(0)).astype(np.int64)
        Mz = np.asarray(M, f32)[vi, ui]
        Nw = np.asarray(N, f32)[vi, ui]
        ok &= (Mz > f32(0)) & ((Nw[:, 0] != 0) | (Nw[:, 1] != 0) | (Nw[:, 2] != 0))
        n = [(Rm[3 * i] * Nw[:, 0] + Rm[3 * i + 1] * Nw[:, 1]) + Rm[3 * i + 2] * Nw[:, 2] for i in range(3)]
        ok &= ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) <= f32(NORMAL_MAX)
        umf, vmf = ui.astype(f32), vi.astype(f32)
        pm = [((umf - cx) * inv_fx) * Mz, ((vmf - cy) * inv_fy) * Mz, Mz]
        e = [q[i] - pm[i] for i in range(3)]
        ok &= ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= cfg.dist_max * cfg.dist_max
        ok &= ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) <= cfg.reach * cfg.reach
        r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        c = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0]]
        J = np.stack(c + n, axis=1)
        J = np.where(ok[:, None], J, f32(0))
        r = np.where(ok, r, f32(0))
    return ok, J, r, ui, vi


def quantise(J, r, count):
    """Rule 4: the 29 int64 sums of the fp32 rows J [n, 6] and r [n]; `count` is the number of correspondences."""
    S = np.zeros(N_TERMS, np.int64)
    J64, r64 = J.astype(np.float64), r.astype(np.float64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            S[k] = np.rint((J64[:, i] * J64[:, j]) * SCALE_A).astype(np.int64).sum()
            k += 1
    for i in range(6):
        S[21 + i] = np.rint((J64[:, i] * r64) * SCALE_B).astype(np.int64).sum()
    S[27] = np.rint((r64 * r64) * SCALE_R).astype(np.int64).sum()
    S[28] = count
    return S


def system(cfg, D, M, N, Trel, Rm, stride):
    """The 29 integers of one accumulation at Trel (12 doubles) on the level of `stride`: aria_icp_debug_system_device."""
    ok, J, r, _, _ = jacobians(cfg, D, M, N, Trel, Rm, stride)
    return quantise(J, r, int(ok.sum()))


# ---- rule 5: the solve -----------------------------------------------------------------------------------------------------
Step = namedtuple("Step", "lost delta count rms norm pivots")


def solve(cfg, S):
    """Rule 5 on the 29 integers: Step(lost, delta[6] or None, count, rms, |delta|, the pivots reached)."""
    count = int(S[28])
    rms = math.sqrt((float(int(S[27])) / SCALE_R) / float(count)) if count > 0 else 0.0
    if count < cfg.min_corr:
        return Step(True, None, count, rms, 0.0, [])
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = float(int(S[k])) / SCALE_A
            k += 1
    b = [float(int(S[21 + i])) / SCALE_B for i in range(6)]
    thr = cfg.min_pivot * float(count)
    L = [[0.0] * 6 for _ in range(6)]
    pivots = []
    for j in range(6):
        s = A[j][j]
        for m in range(j):
            s = s - L[j][m] * L[j][m]
        pivots.append(s)
        if not (s > thr):
            return Step(True, None, count, rms, 0.0, pivots)
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = A[j][i]
            for m in range(j):
                s = s - L[i][m] * L[j][m]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -b[i]
        for m in range(i):
            s = s - L[i][m] * y[m]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for m in range(i + 1, 6):
            s = s - L[m][i] * x[m]
        x[i] = s / L[i][i]
    nrm = math.sqrt(((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5])
    return Step(False, x, count, rms, nrm, pivots)


def cayley(w):
    """Rule 5: the rotation increment of delta[0:3], 9 floats row-major."""
    a = [0.5 * w[0], 0.5 * w[1], 0.5 * w[2]]
    s = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den = 1.0 + s
    one = 1.0 - s
    K = [0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0]
    R = [0.0] * 9
    for i in range(3):
        for j in range(3):
            if i == j:
                R[3 * i + j] = (one + 2.0 * (a[i] * a[i])) / den
            else:
                R[3 * i + j] = (2.0 * (a[i] * a[j]) + 2.0 * K[3 * i + j]) / den
    return R


def advance(Trel, delta):
    """Trel <- [Rinc | delta[3:6]] o Trel."""
    Ri = cayley(delta[:3])
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (Ri[3 * i] * Trel[j] + Ri[3 * i + 1] * Trel[4 + j]) + Ri[3 * i + 2] * Trel[8 + j]
        out[4 * i + 3] = ((Ri[3 * i] * Trel[3] + Ri[3 * i + 1] * Trel[7]) + Ri[3 * i + 2] * Trel[11]) + delta[3 + i]
    return out


# ---- rules 5 and 6: one frame ------------------------------------------------------------------------------------------------
Track = namedtuple("Track", "T result")


def track(cfg, D, M, N, Tm, T0, trace=None):
    """One frame: Track(T [12] doubles, result RESULT_DTYPE). A non-finite Tm or T0 gives T = None and valid = 0. `trace`, a
    list, receives (level, S, Step) of every accumulation that ran."""
    res = np.zeros((), RESULT_DTYPE)
    Tm = np.asarray(Tm, np.float64).reshape(12)
    T0 = np.asarray(T0, np.float64).reshape(12)
    if not (np.isfinite(Tm).all() and np.isfinite(T0).all()):
        return Track(None, res)
    check_size(D.shape[1], D.shape[0])
    Trel = relative(Tm, T0)
    Rm = model_rotation(Tm)
    lost = False
    for lv, (stride, its) in enumerate(zip(cfg.strides, cfg.iterations)):
        for _ in range(its):
            S = system(cfg, D, M, N, Trel, Rm, stride)
            st = solve(cfg, S)
            if trace is not None:
                trace.append((lv, S, st))
            res["iterations_run"] += 1
            res["n_corr"], res["rms"], res["delta"], res["level"] = st.count, st.rms, st.norm, lv
            if st.lost:
                lost = True
                break
            Trel = advance(Trel, st.delta)
            if st.norm < cfg.eps:
                break
        if lost:
            break
    if lost:
        return Track(T0.copy(), res)
    res["valid"] = 1
    return Track(output_pose(Trel, Tm), res)


def track_batch(cfg, depths, model_depths, model_normals, Tm, T0, mask=None):
    """(tracks, invalid): one Track per frame, None for a frame whose mask byte is 0 (nothing of it is written); invalid is
    True when some unmasked frame had a non-finite Tm or T0 (aria_icp_check then reports ARIA_E_INVALID)."""
    out, invalid = [], False
    for f in range(len(depths)):
        if mask is not None and not mask[f]:
            out.append(None)
            continue
        t = track(cfg, depths[f], model_depths[f], model_normals[f], Tm[f], T0[f])
        invalid |= t.T is None
        out.append(t)
    return out, invalid


def algorithmic_bytes(cfg, width, height, n_frames):
    """The bytes a call must move: per iteration and level pixel 4 of live depth and 4 + 12 of the model, and per frame the
    two poses read (192), the pose written (96) and the record (32)."""
    px = sum(n * ((width + s - 1) // s) * ((height + s - 1) // s) for s, n in zip(cfg.strides, cfg.iterations))
    return (20 * px + 320) * n_frames
