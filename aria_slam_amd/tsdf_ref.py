"""NumPy restatement of the dense depth fusion stage (include/aria_orb_hip.h, "dense depth fusion"): the truncated signed
distance volume that fp32 depth maps are integrated into along a trajectory, and the surface points read back out of it.
The reference has no code for it, so this file IS the definition and the device equals it bit for bit.

Every float operation below is fp32 with one rounding per operation, in the order the header writes it: the operands are
np.float32 arrays or scalars throughout, NumPy contracts nothing, and fp32 division is correctly rounded. Nothing is culled
here: every voxel meets every frame."""
from collections import namedtuple

import numpy as np

VOXEL_DTYPE = np.dtype([("tsdf", "<f4"), ("weight", "<u2"), ("gray", "u1"), ("reserved", "u1")])      # aria_tsdf_voxel, 8 bytes
POINT_DTYPE = np.dtype([("X", "<f4", (3,)), ("gray", "u1"), ("axis", "u1"), ("weight", "<u2")])       # aria_tsdf_point, 16 bytes

EUROC_K = (458.654, 457.296, 367.215, 248.375)
DEFAULTS = dict(dims=(256, 256, 128), voxel=0.05, origin=(-6.4, -6.4, 0.0), trunc=0.20, min_depth=0.3, max_depth=10.0,
                max_weight=64, min_weight=2, K=EUROC_K)

Config = namedtuple("Config", "dims voxel origin trunc min_depth max_depth max_weight min_weight K")

f32 = np.float32


def config(**kw):
    """A Config from DEFAULTS and the overrides; raises ValueError where aria_tsdf_create returns ARIA_E_INVALID."""
    d = dict(DEFAULTS)
    d.update(kw)
    c = Config(dims=tuple(int(v) for v in d["dims"]), voxel=f32(d["voxel"]), origin=tuple(f32(v) for v in d["origin"]),
               trunc=f32(d["trunc"]), min_depth=f32(d["min_depth"]), max_depth=f32(d["max_depth"]),
               max_weight=int(d["max_weight"]), min_weight=int(d["min_weight"]), K=tuple(float(v) for v in d["K"]))
    ok = len(c.dims) == 3 and all(8 <= n <= 1024 and n % 8 == 0 for n in c.dims)
    ok = ok and np.isfinite(c.voxel) and c.voxel > 0 and np.isfinite(c.trunc) and c.trunc > 0
    ok = ok and all(np.isfinite(v) for v in c.origin) and c.min_depth <= c.max_depth
    ok = ok and 1 <= c.max_weight <= 65535 and 1 <= c.min_weight <= 65535 and all(np.isfinite(v) for v in c.K)
    if not ok:
        raise ValueError("invalid TSDF configuration")
    return c


def new_volume(cfg):
    """The cleared volume, indexed [k, j, i]: linear index (k*ny + j)*nx + i, x fastest."""
    nx, ny, nz = cfg.dims
    return np.zeros((nz, ny, nx), VOXEL_DTYPE)


def centres(cfg):
    """c = origin + ((float)i + 0.5f) * voxel per axis: three fp32 vectors (x over i, y over j, z over k)."""
    return tuple(f32(cfg.origin[a]) + (np.arange(cfg.dims[a], dtype=f32) + f32(0.5)) * cfg.voxel for a in range(3))


def integrate(vol, cfg, depth, extrinsics, image=None):
    """Steps 1-8 of one frame into vol (in place). depth: fp32 [H, W]; extrinsics: 12 doubles [R|t] row-major, world to
    camera; image: uint8 [H, W] or None. Returns False, with vol untouched, when an extrinsic is not finite."""
    e64 = np.asarray(extrinsics, np.float64).reshape(12)
    if not np.isfinite(e64).all():
        return False
    with np.errstate(all="ignore"):
        e = e64.astype(f32)
        depth = np.asarray(depth, f32)
        H, W = depth.shape
        fx, fy, cx, cy = (f32(v) for v in cfg.K)
        inv_trunc = f32(1.0) / cfg.trunc
        gx, gy, gz = centres(cfg)
        cX, cY, cZ = gx[None, None, :], gy[None, :, None], gz[:, None, None]
        xc = ((e[0] * cX + e[1] * cY) + e[2] * cZ) + e[3]
        yc = ((e[4] * cX + e[5] * cY) + e[6] * cZ) + e[7]
        zc = ((e[8] * cX + e[9] * cY) + e[10] * cZ) + e[11]
        ok = zc >= cfg.min_depth
        iz = f32(1.0) / zc
        u = (fx * xc) * iz + cx
        v = (fy * yc) * iz + cy
        ur, vr = np.rint(u), np.rint(v)
        ok &= (ur >= f32(0)) & (ur <= f32(W - 1)) & (vr >= f32(0)) & (vr <= f32(H - 1))
        ui = np.where(ok, ur, f32(0)).astype(np.int64)
        vi = np.where(ok, vr, f32(0)).astype(np.int64)
        D = depth[vi, ui]
        ok &= (D >= cfg.min_depth) & (D <= cfg.max_depth)
        sdf = D - zc
        ok &= ~(sdf < -cfg.trunc)
        s = np.minimum(f32(1.0), sdf * inv_trunc)
        w0 = vol["weight"]
        w = w0.astype(f32)
        t = (vol["tsdf"] * w + s) / (w + f32(1.0))
        if image is not None:
            g = np.asarray(image, np.uint8)[vi, ui].astype(np.int64)
            W0 = w0.astype(np.int64)
            gray = (vol["gray"].astype(np.int64) * W0 + g + ((W0 + 1) >> 1)) // (W0 + 1)
            vol["gray"] = np.where(ok, gray, vol["gray"]).astype(np.uint8)
        vol["tsdf"] = np.where(ok, t, vol["tsdf"])
        vol["weight"] = np.where(ok, np.minimum(w0.astype(np.int64) + 1, cfg.max_weight), w0).astype(np.uint16)
    return True


def integrate_batch(vol, cfg, depths, extrinsics, frame_mask=None, images=None):
    """The frames in ascending order; a frame whose mask byte is 0 is skipped. Returns True when some unmasked frame had a
    non-finite extrinsic (that frame is skipped: aria_tsdf_check then reports ARIA_E_INVALID)."""
    invalid = False
    for f in range(len(depths)):
        if frame_mask is not None and not frame_mask[f]:
            continue
        invalid |= not integrate(vol, cfg, depths[f], extrinsics[f], None if images is None else images[f])
    return invalid


def extract(vol, cfg, cap=None, min_weight=None):
    """(points, total): the surface points in canonical order (voxel a in ascending linear index, then axis 0, 1, 2), cut
    to the first min(total, cap)."""
    mw = cfg.min_weight if min_weight is None else min_weight
    nx, ny, nz = cfg.dims
    gx, gy, gz = centres(cfg)
    t, w, g = vol["tsdf"], vol["weight"], vol["gray"]
    recs = []
    with np.errstate(all="ignore"):
        for axis in range(3):
            sa = [slice(None)] * 3
            sb = [slice(None)] * 3
            sa[2 - axis], sb[2 - axis] = slice(0, -1), slice(1, None)
            sa, sb = tuple(sa), tuple(sb)
            ta, tb = t[sa], t[sb]
            hit = (w[sa] >= mw) & (w[sb] >= mw) & ((ta < 0) != (tb < 0))
            k, j, i = np.nonzero(hit)
            ta, tb = ta[hit], tb[hit]
            alpha = ta / (ta - tb)
            p = np.zeros(len(k), POINT_DTYPE)
            X = np.stack([gx[i], gy[j], gz[k]], axis=1)
            X[:, axis] = X[:, axis] + alpha * cfg.voxel
            p["X"] = X
            p["gray"] = np.where(alpha < f32(0.5), g[sa][hit], g[sb][hit])
            p["axis"] = axis
            p["weight"] = np.minimum(w[sa][hit], w[sb][hit])
            recs.append(((k.astype(np.int64) * ny + j) * nx + i, p))
    lin = np.concatenate([r[0] for r in recs])
    pts = np.concatenate([r[1] for r in recs])
    order = np.lexsort((pts["axis"], lin))
    pts = pts[order]
    total = len(pts)
    return (pts if cap is None else pts[:min(total, cap)]).copy(), total


def volume_bytes(nx, ny, nz):
    return 8 * nx * ny * nz


def algorithmic_bytes(nx, ny, nz, width, height, n_frames):
    """One call: every voxel record read and written once (16 B), every depth pixel read once per frame (4 B)."""
    return 16 * nx * ny * nz + 4 * width * height * n_frames
