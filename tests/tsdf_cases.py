"""Shared inputs of the depth fusion tests (test_tsdf_host.py, test_tsdf_kernel_emulation.py, test_gpu_tsdf.py): analytic
depth renders of a plane plus a sphere, the shapes (a)-(h) the device tests run, and the restatement's results on them
(aria_slam_amd/tsdf_ref.py), computed once per process and handed out read-only."""
import functools

import numpy as np

from aria_slam_amd import tsdf_ref as R

# the scene: renders of 80 x 60, a volume of 32 x 24 x 16 voxels of 0.1 m around a plane at z = 2.4 and a sphere
W, H = 80, 60
K = (60.0, 60.0, 39.5, 29.5)
DIMS, VOXEL, TRUNC = (32, 24, 16), 0.1, 0.3
ORIGIN = (-1.6, -1.2, 1.2)
PLANE_Z = 2.4
SPHERE_C, SPHERE_R = (0.1, -0.05, 1.9), 0.45
POSES = ((0.0, 0.0), (0.15, -0.3), (-0.2, 0.35))                     # (yaw in rad, x offset of the camera centre in m)
GUARD = 0x5A

# shape (b): an 8 x 8 x 8 volume under a 5 x 3 depth map, every layout padded
SMALL_W, SMALL_H = 5, 3
SMALL_K = (2.0, 2.0, 2.0, 1.0)
SMALL_DEPTH_PITCH, SMALL_DEPTH_STRIDE = 7, 7 * 3 + 4
SMALL_IMG_PITCH, SMALL_IMG_STRIDE = 6, 6 * 3 + 5


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def scene_config(**kw):
    d = dict(dims=DIMS, voxel=VOXEL, origin=ORIGIN, trunc=TRUNC, K=K)
    d.update(kw)
    return R.config(**d)


def small_config(**kw):
    d = dict(dims=(8, 8, 8), voxel=0.25, origin=(-1.0, -1.0, 0.5), trunc=0.5, K=SMALL_K, min_depth=0.5, max_depth=3.0, min_weight=1)
    d.update(kw)
    return R.config(**d)


def pose(yaw=0.0, x=0.0, pitch=0.0, y=0.0, z=0.0):
    """World-to-camera [R|t] as 12 doubles for a camera at (x, y, z) turned by yaw about the y axis, then pitch about x."""
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rcw = (Ry @ Rx).T                                                # the camera's axes in the world are the columns of Ry Rx
    t = -Rcw @ np.array([x, y, z], np.float64)
    return np.concatenate([Rcw, t[:, None]], axis=1).reshape(12)


@functools.lru_cache(maxsize=None)
def render(yaw=0.0, x=0.0, pitch=0.0, y=0.0, z=0.0, plane=PLANE_Z, sphere=True):
    """(depth fp32 [H, W], gray uint8 [H, W]) of the plane z = `plane` and the sphere seen from pose(...): the z coordinate
    in the camera of the nearer hit along each pixel's ray, 0 where there is none."""
    e = pose(yaw, x, pitch, y, z).reshape(3, 4)
    Rcw, t = e[:, :3], e[:, 3]
    o = -Rcw.T @ t
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], axis=-1)
    d = dc @ Rcw                                                     # rows: Rcw^T dc
    with np.errstate(all="ignore"):
        s = np.where(d[..., 2] > 1e-9, (plane - o[2]) / d[..., 2], np.inf)
        s[s <= 0] = np.inf
        if sphere:
            oc = o - np.array(SPHERE_C)
            a = (d * d).sum(-1)
            b = 2.0 * (d @ oc)
            c = oc @ oc - SPHERE_R ** 2
            disc = b * b - 4 * a * c
            s1 = (-b - np.sqrt(disc)) / (2 * a)
            s1 = np.where((disc > 0) & (s1 > 0), s1, np.inf)
            s = np.minimum(s, s1)
    depth = np.where(np.isfinite(s), s, 0.0).astype(np.float32)
    gray = ((u * 3 + v * 5 + 17 * np.floor(depth * 8)) % 256).astype(np.uint8)
    return _ro(depth, gray)


@functools.lru_cache(maxsize=None)
def scene_frames():
    """Shape (a): (depths [3, H, W], images [3, H, W], extrinsics [3, 12]) of the three poses."""
    r = [render(yaw, x) for yaw, x in POSES]
    return _ro(np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.stack([pose(yaw, x) for yaw, x in POSES]))


@functools.lru_cache(maxsize=None)
def five_frames():
    """Shapes (c), (d): five poses along a short arc, with their renders."""
    ps = [(0.04 * k - 0.08, 0.1 * k - 0.2) for k in range(5)]
    r = [render(yaw, x) for yaw, x in ps]
    return _ro(np.stack([a[0] for a in r]), np.stack([a[1] for a in r]), np.stack([pose(yaw, x) for yaw, x in ps]))


FRUSTUM_POSES = {
    "inside": dict(x=0.2, y=0.1, z=1.7),                             # the camera sits inside the volume
    "half_behind": dict(z=2.0, yaw=0.1),                             # the camera plane cuts the volume
    "outside": dict(yaw=np.pi),                                      # looks away: no voxel is in view
    "yaw_pitch": dict(yaw=0.5, pitch=0.5, x=-1.2, y=1.0, z=0.2),     # tiles straddle all four image borders
    "narrow": dict(yaw=0.3, pitch=-0.1, x=-0.5),                     # a 20 x 15 view: whole tiles lie beside the frustum
}
NARROW_SIZE, NARROW_K = (20, 15), (60.0, 60.0, 9.5, 7.0)


def frustum_view(name):
    """(W, H), K of a frustum pose."""
    return (NARROW_SIZE, NARROW_K) if name == "narrow" else ((W, H), K)


@functools.lru_cache(maxsize=None)
def frustum_frame(name):
    """Shape (e): (depth, image, extrinsics). The depth map is a plane far enough to lie in front of every voxel in view, so
    that every voxel that projects into the image is touched."""
    kw = FRUSTUM_POSES[name]
    (w, h), _ = frustum_view(name)
    depth = np.full((h, w), 2.0, np.float32)
    depth[::7, ::5] = 0.0
    gray = render()[1][:h, :w]
    return _ro(depth.copy(), gray.copy(), pose(**kw))


@functools.lru_cache(maxsize=None)
def small_frames():
    """Shape (b): three 5 x 3 depth maps with 0, negatives, NaN, +Inf and values one ulp outside [min_depth, max_depth]."""
    cfg = small_config()
    lo, hi = cfg.min_depth, cfg.max_depth
    d = np.array([[[1.0, 1.5, 2.0, 2.5, 3.0], [0.0, -1.0, np.nan, np.inf, 1.25], [lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(9)), 1.75]],
                  [[np.nan, 1.1, 0.0, 1.6, -0.0], [2.2, 2.2, 2.2, -np.inf, 0.75], [1.0, 1.0, np.inf, 1.0, 2.75]],
                  [[1.9, 1.9, 1.9, 1.9, 1.9], [1.4, np.nan, 1.4, 0.0, 1.4], [hi, lo, -2.0, 1.0, 1.0]]], np.float32)
    img = (np.arange(3 * SMALL_H * SMALL_W).reshape(3, SMALL_H, SMALL_W) * 37 % 256).astype(np.uint8)
    ext = np.stack([pose(), pose(yaw=0.2, x=0.1), pose(yaw=-0.15, x=-0.2, pitch=0.1)])
    return _ro(d, img, ext)


N_MANY = 70


@functools.lru_cache(maxsize=None)
def many_frames():
    """70 frames on shape (b)'s volume (three words of the tile masks, the last with 6 bits): its depth maps and images in turn
    under poses spread over +-0.6 rad of yaw and pitch, every seventh one looking away."""
    d, im, _ = small_frames()
    rng = np.random.default_rng(70)
    ext = np.stack([pose(yaw=np.pi if k % 7 == 3 else rng.uniform(-0.6, 0.6), pitch=rng.uniform(-0.6, 0.6), x=rng.uniform(-0.5, 0.5),
                         y=rng.uniform(-0.3, 0.3), z=rng.uniform(-0.4, 0.2)) for k in range(N_MANY)])
    idx = np.arange(N_MANY) % 3
    return _ro(np.ascontiguousarray(d[idx]), np.ascontiguousarray(im[idx]), ext)


def ref_many():
    def build():
        cfg = small_config(max_weight=20)
        d, im, e = many_frames()
        vol, _ = ref_integrated(cfg, d, e, im)
        return cfg, vol, R.extract(vol, cfg)[0]
    return ref("many", build)


def padded(frames, pitch, stride, dtype, fill):
    """n frames (H, W) laid out with `pitch` elements per row and `stride` elements per frame, padding = fill."""
    n, (h, w) = len(frames), frames[0].shape
    buf = np.full((n, stride), fill, dtype)
    for k, f in enumerate(frames):
        buf[k, :pitch * h].reshape(h, pitch)[:, :w] = f
    return buf


_cache = {}


def ref(name, build):
    """The restatement's result under `name`, computed by build() once per process; arrays come back read-only."""
    if name not in _cache:
        out = build()
        for a in out if isinstance(out, tuple) else (out,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


def ref_integrated(cfg, depths, extrinsics, images=None, mask=None):
    """(volume, invalid) of the restatement, not cached."""
    vol = R.new_volume(cfg)
    invalid = R.integrate_batch(vol, cfg, depths, extrinsics, mask, images)
    return vol, invalid


def ref_scene():
    """Shape (a): (cfg, volume, points) of the three-pose scene with images."""
    def build():
        cfg = scene_config()
        d, im, e = scene_frames()
        vol, _ = ref_integrated(cfg, d, e, im)
        return cfg, vol, R.extract(vol, cfg)[0]
    return ref("scene", build)


def ref_small():
    def build():
        cfg = small_config()
        d, im, e = small_frames()
        vol, _ = ref_integrated(cfg, d, e, im)
        return cfg, vol, R.extract(vol, cfg)[0]
    return ref("small", build)


def ref_frustum(name):
    def build():
        cfg = scene_config(min_weight=1, K=frustum_view(name)[1])
        d, im, e = frustum_frame(name)
        vol, _ = ref_integrated(cfg, [d], [e], [im])
        return cfg, vol, R.extract(vol, cfg)[0]
    return ref("frustum_" + name, build)


def ref_five(**kw):
    def build():
        cfg = scene_config(**kw)
        d, im, e = five_frames()
        vol, _ = ref_integrated(cfg, d, e, im)
        return cfg, vol, R.extract(vol, cfg)[0]
    return ref("five_%r" % sorted(kw.items()), build)


def surface_distance(X):
    """Distance of points [n, 3] to the nearer of the plane and the sphere."""
    X = np.asarray(X, np.float64)
    return np.minimum(np.abs(X[:, 2] - PLANE_Z), np.abs(np.linalg.norm(X - np.array(SPHERE_C), axis=1) - SPHERE_R))
