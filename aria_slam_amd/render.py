"""Ray casting of the volume on the device (include/aria_orb_hip.h, "ray casting of the volume"): predicted fp32 depth maps,
world-frame normals, the fused gray and a head-light shade of a TSDF volume at a batch of poses. The reference has no code
for it; aria_slam_amd.ray_ref is the definition and the device equals it bit for bit. The stage owns no volume: update()
hands it the records of a HipTsdfVolume where they lie in HBM.

As with the other stages, the handle's own stream is non-blocking: a volume filled on another stream (the volume handle's
own) must be synchronised before update(), or the renderer must be created on that stream."""
import numpy as np

from . import _lib, ray_ref
from ._handle import StageHandle
from ._lib import RAY_VIEW_DTYPE, check
from .frontend import _ptr


class HipVolumeRenderer(StageHandle):
    """Binding of aria_ray_t. dims, voxel, origin and min_weight are those of the volume that is cast; K = (fx, fy, cx, cy)
    of the views (default EuRoC cam0); near, far and step (default: 0.3, 10 and 0.05) in metres of camera depth."""

    _prefix, _config = "ray", _lib.RayConfig

    def __init__(self, dims=None, voxel=None, origin=None, min_weight=None, near=None, far=None, step=None, skip=None, K=None,
                 stream=None, device=0):
        cfg = self._default_config(device, stream)
        if dims is not None:
            cfg.nx, cfg.ny, cfg.nz = dims
        if origin is not None:
            cfg.origin[0], cfg.origin[1], cfg.origin[2] = (float(v) for v in origin)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        for name, v in (("voxel", voxel), ("min_weight", min_weight), ("near", near), ("far", far), ("step", step), ("skip", skip)):
            if v is not None:
                setattr(cfg, name, v)
        self._create(cfg)

    @classmethod
    def from_volume(cls, vol, **kw):
        """A renderer of the geometry (dims, voxel, origin), min_weight and intrinsics of a HipTsdfVolume, on its device,
        with step = voxel unless given, already updated from the volume. The volume's stream is synchronised first."""
        c = vol.config
        d = dict(dims=(c.nx, c.ny, c.nz), voxel=c.voxel, origin=tuple(c.origin), min_weight=c.min_weight, step=c.voxel,
                 K=(c.fx, c.fy, c.cx, c.cy), device=c.device)
        d.update(kw)
        r = cls(**d)
        vol.check()
        r.update(vol)
        return r

    @property
    def ref_config(self):
        """The configuration as ray_ref.Config."""
        c = self.config
        return ray_ref.config(dims=(c.nx, c.ny, c.nz), voxel=c.voxel, origin=tuple(c.origin), min_weight=c.min_weight, near=c.near,
                              far=c.far, step=c.step, skip=c.skip, K=(c.fx, c.fy, c.cx, c.cy))

    def update(self, vol):
        """aria_ray_update_from_volume_device from a HipTsdfVolume of this geometry (or the device address of its records):
        remembers the address and rebuilds the skip words; enqueued on this handle's stream. The object is held until the
        next update or close(), so a tensor passed here cannot be freed under the handle. Call it again after the volume
        changed."""
        if hasattr(vol, "device_voxels"):
            c, v = self.config, vol.config
            if (c.nx, c.ny, c.nz, c.voxel, tuple(c.origin)) != (v.nx, v.ny, v.nz, v.voxel, tuple(v.origin)):
                raise ValueError("the volume has another geometry (dims, voxel or origin) than the renderer")
            ptr = vol.device_voxels()
        else:
            ptr = _ptr(vol)
        check(self._L.aria_ray_update_from_volume_device(self._h, ptr), "aria_ray_update_from_volume_device")
        self._records = vol                                          # the handle holds their address: keep them alive

    def close(self):
        super().close()
        self._records = None

    def cast_batch_device(self, d_extrinsics, n_views, width, height, d_depth=None, d_normal=None, d_gray=None, d_shade=None,
                          d_views=None, d_view_mask=None, depth_stride=None, depth_pitch=None, normal_stride=None, normal_pitch=None,
                          gray_stride=None, gray_pitch=None, shade_stride=None, shade_pitch=None):
        """aria_ray_cast_batch_device: device pointers (torch tensors or ints), None = that plane is not written. Pitches
        default to the width and strides to a dense view; all in elements (the normals: stride in floats, pitch in pixels).
        Enqueued on the handle's stream; check() synchronises and reports a non-finite view."""
        def layout(stride, pitch, per):
            pitch = width if pitch is None else pitch
            return (per * pitch * height if stride is None else stride), pitch
        ds, dp = layout(depth_stride, depth_pitch, 1)
        ns, np_ = layout(normal_stride, normal_pitch, 3)
        gs, gp = layout(gray_stride, gray_pitch, 1)
        ss, sp = layout(shade_stride, shade_pitch, 1)
        check(self._L.aria_ray_cast_batch_device(self._h, _ptr(d_extrinsics), _ptr(d_view_mask), n_views, width, height, _ptr(d_depth),
                                                 ds, dp, _ptr(d_normal), ns, np_, _ptr(d_gray), gs, gp, _ptr(d_shade), ss, sp,
                                                 _ptr(d_views)), "aria_ray_cast_batch_device")

    def cast(self, extrinsics, width, height, planes=15):
        """One view into host arrays; blocks. Returns ray_ref.Cast(depth, normal, gray, shade, view); a plane whose
        ARIA_RAY_* bit is not in `planes` is None. A non-finite extrinsic raises AriaError (ARIA_E_INVALID)."""
        e = np.ascontiguousarray(np.asarray(extrinsics, np.float64).reshape(-1)[:12])
        if e.size != 12:
            raise ValueError("extrinsics are 12 doubles [R|t], row-major")
        depth = np.zeros((height, width), np.float32) if planes & _lib.RAY_DEPTH else None
        normal = np.zeros((height, width, 3), np.float32) if planes & _lib.RAY_NORMAL else None
        gray = np.zeros((height, width), np.uint8) if planes & _lib.RAY_GRAY else None
        shade = np.zeros((height, width), np.uint8) if planes & _lib.RAY_SHADE else None
        view = np.zeros(1, RAY_VIEW_DTYPE)
        p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
        check(self._L.aria_ray_cast(self._h, e.ctypes.data, width, height, p(depth), p(normal), p(gray), p(shade), view.ctypes.data),
              "aria_ray_cast")
        return ray_ref.Cast(depth, normal, gray, shade, view[0])


def write_depth_pgm(path, depth):
    """A depth map as a binary 16-bit PGM in millimetres, most significant byte first, 0 = no hit, 65535 = 65.535 m or more:
    the file euroc_frontend --render writes as PREFIX_<frame>_depth.pgm."""
    d = np.asarray(depth, np.float32)
    mm = np.clip(np.rint(d.astype(np.float64) * 1000.0), 0, 65535).astype(">u2")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (d.shape[1], d.shape[0]))
        f.write(mm.tobytes())


def write_gray_pgm(path, image):
    """An 8-bit plane (shade or gray) as a binary PGM: the file euroc_frontend --render writes as PREFIX_<frame>_shade.pgm."""
    a = np.ascontiguousarray(image, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())


def read_pgm(path):
    """A binary PGM of either depth as a uint8 or uint16 array [H, W]."""
    raw = open(path, "rb").read()
    fields, pos = [], 0
    while len(fields) < 4:
        end = pos
        while raw[end:end + 1] not in (b" ", b"\n", b"\t", b"\r"):
            end += 1
        if end > pos:
            fields.append(raw[pos:end])
        pos = end + 1
    if fields[0] != b"P5":
        raise ValueError("not a binary PGM")
    w, h, maxval = int(fields[1]), int(fields[2]), int(fields[3])
    return np.frombuffer(raw, ">u2" if maxval > 255 else "u1", w * h, pos).reshape(h, w)


def algorithmic_bytes(width, height, n_views, planes=15):
    return _lib.load_library().aria_ray_algorithmic_bytes(width, height, n_views, planes)
