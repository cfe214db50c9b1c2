"""Dense depth fusion on the device (include/aria_orb_hip.h, "dense depth fusion"): the fp32 depth maps of HipDenseStereo
integrated along the trajectory into one truncated signed distance volume kept in HBM, and the surface points read back
out of it. The reference has no code for it; aria_slam_amd.tsdf_ref is the definition and the device equals it bit for bit.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on another stream (torch's
default stream, another handle's) must be synchronised before a *_device call, or the handle must be created on that
stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import TSDF_POINT_DTYPE, TSDF_VOXEL_DTYPE, check
from .frontend import _ptr
from .mapper import ply_text


class HipTsdfVolume(StageHandle):
    """Binding of aria_tsdf_t. dims = (nx, ny, nz), each a multiple of 8; K = (fx, fy, cx, cy) of the depth maps (default
    EuRoC cam0); origin = the world corner of voxel (0, 0, 0)."""

    _prefix, _config = "tsdf", _lib.TsdfConfig

    def __init__(self, dims=None, voxel=None, origin=None, trunc=None, min_depth=None, max_depth=None, max_weight=None,
                 min_weight=None, K=None, stream=None, device=0):
        cfg = self._default_config(device, stream)
        if dims is not None:
            cfg.nx, cfg.ny, cfg.nz = dims
        if origin is not None:
            cfg.origin[0], cfg.origin[1], cfg.origin[2] = (float(v) for v in origin)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        for name, v in (("voxel", voxel), ("trunc", trunc), ("min_depth", min_depth), ("max_depth", max_depth),
                        ("max_weight", max_weight), ("min_weight", min_weight)):
            if v is not None:
                setattr(cfg, name, v)
        self._create(cfg)

    @property
    def dims(self):
        return (self.config.nx, self.config.ny, self.config.nz)

    def clear(self):
        """Every byte of the volume back to zero; enqueued."""
        check(self._L.aria_tsdf_clear(self._h), "aria_tsdf_clear")

    def integrate(self, depth, extrinsics, image=None):
        """One frame from host arrays; blocks. depth: fp32 [H, W]; extrinsics: 12 doubles [R|t] (or a 4x4 / 3x4 matrix),
        world to camera; image: uint8 [H, W] or None."""
        d = np.asarray(depth, np.float32)
        if d.ndim != 2:
            raise ValueError("the depth map must be 2-D")
        if d.strides[1] != 4 or d.strides[0] % 4 or d.strides[0] < 4 * d.shape[1]:
            d = np.ascontiguousarray(d)
        e = np.ascontiguousarray(np.asarray(extrinsics, np.float64).reshape(-1)[:12])
        if e.size != 12:
            raise ValueError("extrinsics are 12 doubles [R|t], row-major")
        im = None
        if image is not None:
            im = np.asarray(image, np.uint8)
            if im.shape != d.shape:
                raise ValueError("the image must have the depth map's size")
            if im.strides[1] != 1 or im.strides[0] < im.shape[1]:
                im = np.ascontiguousarray(im)
        h, w = d.shape
        check(self._L.aria_tsdf_integrate(self._h, d.ctypes.data, w, h, d.strides[0] // 4, e.ctypes.data,
                                          im.ctypes.data if im is not None else None, im.strides[0] if im is not None else 0),
              "aria_tsdf_integrate")

    def integrate_batch_device(self, d_depth, width, height, d_extrinsics, n_frames, d_frame_mask=None, d_img=None, depth_stride=None,
                               depth_pitch=None, img_stride=None, img_pitch=None):
        """aria_tsdf_integrate_batch_device: device pointers (torch tensors or ints). Pitches default to the width and
        strides to pitch * height; those of the depth maps are in elements. Enqueued on the handle's stream; check()
        synchronises and reports deferred errors."""
        depth_pitch = width if depth_pitch is None else depth_pitch
        img_pitch = width if img_pitch is None else img_pitch
        depth_stride = depth_pitch * height if depth_stride is None else depth_stride
        img_stride = img_pitch * height if img_stride is None else img_stride
        check(self._L.aria_tsdf_integrate_batch_device(self._h, _ptr(d_depth), depth_stride, depth_pitch, width, height,
                                                       _ptr(d_extrinsics), _ptr(d_frame_mask), _ptr(d_img), img_stride, img_pitch,
                                                       n_frames), "aria_tsdf_integrate_batch_device")

    def extract_points_device(self, d_points, cap, d_count):
        """aria_tsdf_extract_points_device: cap TSDF_POINT_DTYPE records at d_points, the int64 total at d_count. Enqueued."""
        check(self._L.aria_tsdf_extract_points_device(self._h, _ptr(d_points), cap, _ptr(d_count)), "aria_tsdf_extract_points_device")

    def count_points(self):
        """The number of surface points the volume holds; blocks."""
        total = C.c_int64()
        rc = self._L.aria_tsdf_extract_points(self._h, None, 0, C.byref(total))
        if rc not in (_lib.ARIA_OK, _lib.ARIA_E_OUTPUT_TOO_SMALL):
            check(rc, "aria_tsdf_extract_points")
        return total.value

    def extract_points(self, cap=None):
        """The surface points in canonical order as TSDF_POINT_DTYPE records; blocks. With a `cap` smaller than the total the
        first cap points come back together with the total: (points, total); without one, all points."""
        n = self.count_points() if cap is None else cap
        pts = np.zeros(n, TSDF_POINT_DTYPE)
        total = C.c_int64()
        rc = self._L.aria_tsdf_extract_points(self._h, pts.ctypes.data if n else None, n, C.byref(total))
        if cap is None:
            check(rc, "aria_tsdf_extract_points")
            return pts
        if rc != _lib.ARIA_E_OUTPUT_TOO_SMALL:
            check(rc, "aria_tsdf_extract_points")
        return pts[:min(n, total.value)], total.value

    def voxels(self):
        """The whole volume as TSDF_VOXEL_DTYPE records [nz, ny, nx]; blocks."""
        nx, ny, nz = self.dims
        return self.read_box(0, 0, 0, nx, ny, nz)

    def device_voxels(self):
        """The device address of the volume (aria_tsdf_device_voxels)."""
        return self._L.aria_tsdf_device_voxels(self._h)

    def read_box(self, i0, j0, k0, ni, nj, nk):
        """The records of [i0, i0+ni) x [j0, j0+nj) x [k0, k0+nk) as an array [nk, nj, ni]; blocks."""
        out = np.zeros((max(nk, 0), max(nj, 0), max(ni, 0)), TSDF_VOXEL_DTYPE)
        check(self._L.aria_tsdf_read_box(self._h, i0, j0, k0, ni, nj, nk, out.ctypes.data), "aria_tsdf_read_box")
        return out

    def export_ply(self, path):
        """The surface points in the PLY header and vertex format HipMapper.export_ply writes (r = g = b = gray)."""
        with open(path, "w") as f:
            f.write(ply_text(self.extract_points()))


def volume_bytes(nx, ny, nz):
    return _lib.load_library().aria_tsdf_volume_bytes(nx, ny, nz)


def algorithmic_bytes(nx, ny, nz, width, height, n_frames):
    return _lib.load_library().aria_tsdf_algorithmic_bytes(nx, ny, nz, width, height, n_frames)
