"""NumPy restatement of the ray casting stage (include/aria_orb_hip.h, "ray casting of the volume"): a ray per pixel marched
through the truncated signed distance volume of the dense depth fusion, the zero crossing refined on the trilinear
interpolant, and that interpolant differentiated: a predicted depth map, world-frame normals, the fused gray and a head-light
shade per view, plus a 16-byte record per view. The reference has no code for it, so this file IS the definition and the
device equals it bit for bit.

Every float operation below is fp32 with one rounding per operation, in the order the header writes it: the operands are
np.float32 arrays or scalars throughout, NumPy contracts nothing, and fp32 division and square root are correctly rounded.
Nothing is clipped and nothing is skipped here: every ray meets every sample k = 0 .. n_steps - 1 until its walk ends. The
records' tsdf values must not be infinite (rule 1): a NaN depth and the `nearest` of its view are not defined."""
from collections import namedtuple

import numpy as np

from .tsdf_ref import EUROC_K, VOXEL_DTYPE  # noqa: F401  (VOXEL_DTYPE: the records this stage reads)

VIEW_DTYPE = np.dtype([("n_hit", "<i4"), ("n_ended", "<i4"), ("nearest", "<f4"), ("valid", "<i4")])  # aria_ray_view, 16 bytes

DEFAULTS = dict(dims=(256, 256, 128), voxel=0.05, origin=(-6.4, -6.4, 0.0), min_weight=2, near=0.3, far=10.0, step=0.05,
                skip=1, K=EUROC_K)
MAX_STEPS = 8192

Config = namedtuple("Config", "dims voxel origin min_weight near far step skip K")
Cast = namedtuple("Cast", "depth normal gray shade view")

f32 = np.float32


def n_steps(cfg):
    """(int)floorf((far - near) / step) + 1 in fp32."""
    return int(np.floor((cfg.far - cfg.near) / cfg.step)) + 1


def config(**kw):
    """A Config from DEFAULTS and the overrides; raises ValueError where aria_ray_create returns ARIA_E_INVALID."""
    d = dict(DEFAULTS)
    d.update(kw)
    c = Config(dims=tuple(int(v) for v in d["dims"]), voxel=f32(d["voxel"]), origin=tuple(f32(v) for v in d["origin"]),
               min_weight=int(d["min_weight"]), near=f32(d["near"]), far=f32(d["far"]), step=f32(d["step"]), skip=int(d["skip"]),
               K=tuple(float(v) for v in d["K"]))
    ok = len(c.dims) == 3 and all(8 <= n <= 1024 and n % 8 == 0 for n in c.dims)
    ok = ok and np.isfinite(c.voxel) and c.voxel > 0 and all(np.isfinite(v) for v in c.origin)
    ok = ok and 1 <= c.min_weight <= 65535 and c.skip in (0, 1) and all(np.isfinite(v) for v in c.K)
    ok = ok and np.isfinite(c.near) and np.isfinite(c.far) and np.isfinite(c.step) and c.near > 0 and c.far >= c.near and c.step > 0
    if ok:
        with np.errstate(all="ignore"):
            q = np.floor((c.far - c.near) / c.step)
        ok = bool(np.isfinite(q)) and 1 <= int(q) + 1 <= MAX_STEPS
    if not ok:
        raise ValueError("invalid ray casting configuration")
    return c


def from_tsdf(tcfg, **kw):
    """The Config that casts a volume of the tsdf_ref.Config `tcfg`: its geometry, min_weight and intrinsics, step = voxel."""
    d = dict(dims=tcfg.dims, voxel=tcfg.voxel, origin=tcfg.origin, min_weight=tcfg.min_weight, K=tcfg.K, step=tcfg.voxel)
    d.update(kw)
    return config(**d)


def _lerp(a, b, w):
    return a + w * (b - a)


def _grid(cfg, og, dg, z):
    """Rule 4: g_a = og_a + z * dg_a per axis."""
    return [og[a] + z * dg[a] for a in range(3)]


def _cell(vol, cfg, g):
    """Rule 6 at the grid positions g (three fp32 vectors): (defined, t[8] indexed x + 2y + 4z, f[3])."""
    t_, w_ = vol["tsdf"], vol["weight"]
    b = [np.floor(g[a]) for a in range(3)]
    f = [g[a] - b[a] for a in range(3)]
    ok = np.ones(g[0].shape, bool)
    for a in range(3):
        ok &= (b[a] >= f32(0)) & (b[a] + f32(1.0) <= f32(cfg.dims[a] - 1))
    bi = [np.where(ok, b[a], f32(0)).astype(np.int64) for a in range(3)]
    t = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                idx = (bi[2] + dz, bi[1] + dy, bi[0] + dx)
                ok &= w_[idx] >= cfg.min_weight
                t.append(t_[idx])
    return ok, t, f


def _interp(t, f):
    """c00, c10, c01, c11, c0, c1, T of rule 6."""
    c00, c10 = _lerp(t[0], t[1], f[0]), _lerp(t[2], t[3], f[0])
    c01, c11 = _lerp(t[4], t[5], f[0]), _lerp(t[6], t[7], f[0])
    c0, c1 = _lerp(c00, c10, f[1]), _lerp(c01, c11, f[1])
    return c00, c10, c01, c11, c0, c1, _lerp(c0, c1, f[2])


def cast(vol, cfg, extrinsics, W, H, stats=None):
    """One view: Cast(depth fp32 [H, W], normal fp32 [H, W, 3], gray uint8 [H, W], shade uint8 [H, W], view VIEW_DTYPE).
    vol: VOXEL_DTYPE [nz, ny, nx]; extrinsics: 12 doubles [R|t] row-major, world to camera. A non-finite extrinsic gives
    zeros and valid = 0. `stats`, a dict, receives the branch counts of rules 7 and 9."""
    depth = np.zeros((H, W), f32)
    normal = np.zeros((H, W, 3), f32)
    gray = np.zeros((H, W), np.uint8)
    shade = np.zeros((H, W), np.uint8)
    view = np.zeros((), VIEW_DTYPE)
    e64 = np.asarray(extrinsics, np.float64).reshape(12)
    if not np.isfinite(e64).all():
        return Cast(depth, normal, gray, shade, view)
    view["valid"] = 1
    nx, ny, nz = cfg.dims
    mw = cfg.min_weight
    t_, w_, g_ = vol["tsdf"], vol["weight"], vol["gray"]
    with np.errstate(all="ignore"):
        e = e64.astype(f32)
        R = [[e[0], e[1], e[2]], [e[4], e[5], e[6]], [e[8], e[9], e[10]]]
        t = [e[3], e[7], e[11]]
        inv_voxel = f32(1.0) / cfg.voxel
        fx, fy, cx, cy = (f32(v) for v in cfg.K)
        inv_fx, inv_fy = f32(1.0) / fx, f32(1.0) / fy
        og = []
        for a in range(3):
            o = -((R[0][a] * t[0] + R[1][a] * t[1]) + R[2][a] * t[2])
            og.append((o - cfg.origin[a]) * inv_voxel - f32(0.5))
        u, v = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
        u, v = u.reshape(-1), v.reshape(-1)
        pa, pb = (u - cx) * inv_fx, (v - cy) * inv_fy
        d = [(R[0][a] * pa + R[1][a] * pb) + R[2][a] for a in range(3)]
        dg = [d[a] * inv_voxel for a in range(3)]

        n = W * H
        done = np.zeros(n, bool)
        hit = np.zeros(n, bool)
        k_end = np.zeros(n, np.int64)
        tA, tB = np.zeros(n, f32), np.zeros(n, f32)
        gA, gB = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        prev_ok = np.zeros(n, bool)                                   # sample k - 1 seen with tsdf >= 0
        prev_t, prev_g = np.zeros(n, f32), np.zeros(n, np.uint8)
        for k in range(n_steps(cfg)):
            z = cfg.near + f32(k) * cfg.step
            r = [np.rint(x) for x in _grid(cfg, og, dg, z)]
            inside = np.ones(n, bool)
            for a in range(3):
                inside &= (r[a] >= f32(0)) & (r[a] <= f32(cfg.dims[a] - 1))
            idx = tuple(np.where(inside, r[a], f32(0)).astype(np.int64) for a in (2, 1, 0))
            tk, gk = t_[idx], g_[idx]
            seen = inside & (w_[idx] >= mw)
            end = ~done & seen & (tk < f32(0))
            hit |= end & prev_ok
            k_end[end] = k
            tA[end], tB[end], gA[end], gB[end] = prev_t[end], tk[end], prev_g[end], gk[end]
            done |= end
            prev_ok, prev_t, prev_g = seen & (tk >= f32(0)), tk, gk
            if done.all():
                break

        view["n_ended"] = int(done.sum())
        view["n_hit"] = int(hit.sum())
        px = np.nonzero(hit)[0]
        if len(px):
            ogp = og
            dgp = [x[px] for x in dg]
            z1 = cfg.near + k_end[px].astype(f32) * cfg.step
            z0 = cfg.near + (k_end[px] - 1).astype(f32) * cfg.step
            ok0, t0, f0 = _cell(vol, cfg, _grid(cfg, ogp, dgp, z0))
            ok1, t1, f1 = _cell(vol, cfg, _grid(cfg, ogp, dgp, z1))
            F0, F1 = _interp(t0, f0)[6], _interp(t1, f1)[6]
            tri = ok0 & ok1 & (F0 >= f32(0)) & (F1 <= f32(0)) & (F0 > F1)
            A, B = np.where(tri, F0, tA[px]), np.where(tri, F1, tB[px])
            alpha = A / (A - B)
            dep = z0 + alpha * cfg.step
            gr = np.where(alpha < f32(0.5), gA[px], gB[px])
            okn, tn, fn = _cell(vol, cfg, _grid(cfg, ogp, dgp, dep))
            c00, c10, c01, c11, c0, c1, _ = _interp(tn, fn)
            Gx = _lerp(_lerp(tn[1] - tn[0], tn[3] - tn[2], fn[1]), _lerp(tn[5] - tn[4], tn[7] - tn[6], fn[1]), fn[2])
            Gy = _lerp(c10 - c00, c11 - c01, fn[2])
            Gz = c1 - c0
            ln = np.sqrt((Gx * Gx + Gy * Gy) + Gz * Gz)
            has = okn & (ln > f32(0))
            nrm = [np.where(has, G / ln, f32(0)) for G in (Gx, Gy, Gz)]
            dp = [x[px] for x in d]
            dl = np.sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2])
            c = np.abs((nrm[0] * dp[0] + nrm[1] * dp[1]) + nrm[2] * dp[2]) / dl
            sh = np.where(has, np.rint(np.fmin(f32(255.0), f32(255.0) * c)), f32(0)).astype(np.uint8)
            depth.reshape(-1)[px] = dep
            normal.reshape(-1, 3)[px] = np.stack(nrm, axis=1)
            gray.reshape(-1)[px] = gr
            shade.reshape(-1)[px] = sh
            view["nearest"] = dep.min()
            if stats is not None:
                stats.update(hits=len(px), trilinear=int(tri.sum()), nearest_voxel=int((~tri).sum()), normals=int(has.sum()),
                             no_normal=int((~has).sum()))
        elif stats is not None:
            stats.update(hits=0, trilinear=0, nearest_voxel=0, normals=0, no_normal=0)
    return Cast(depth, normal, gray, shade, view)


def cast_batch(vol, cfg, extrinsics, W, H, view_mask=None):
    """(casts, invalid): one Cast per view, None for a view whose mask byte is 0 (nothing of it is written, its record
    included); invalid is True when some unmasked view had a non-finite extrinsic (aria_ray_check then reports
    ARIA_E_INVALID)."""
    out, invalid = [], False
    for f in range(len(extrinsics)):
        if view_mask is not None and not view_mask[f]:
            out.append(None)
            continue
        c = cast(vol, cfg, extrinsics[f], W, H)
        invalid |= not int(c.view["valid"])
        out.append(c)
    return out, invalid


def algorithmic_bytes(width, height, n_views, planes):
    """The bytes one cast writes: 4, 12, 1 and 1 per pixel for the planes of the bit set `planes`, and 16 per view."""
    per = 4 * bool(planes & 1) + 12 * bool(planes & 2) + bool(planes & 4) + bool(planes & 8)
    return (per * width * height + 16) * n_views
