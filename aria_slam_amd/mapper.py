"""Two-view triangulation into a point map on the device (include/aria_orb_hip.h, "two-view triangulation and point map"):
the reference's Mapper (src/legacy/Mapper.cpp) -- triangulate, filterOutliers, filterByDistance, exportPLY, exportPCD --
with the map kept in HBM. aria_slam_amd.map_ref restates the stage in NumPy.

As with HipPoseEstimator, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before triangulate_batch_device, or the mapper must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import KP_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE, check
from .frontend import _ptr

PLY_HEADER = ("ply\n"
              "format ascii 1.0\n"
              "element vertex {n}\n"
              "property float x\n"
              "property float y\n"
              "property float z\n"
              "property uchar red\n"
              "property uchar green\n"
              "property uchar blue\n"
              "end_header\n")
PCD_HEADER = ("# .PCD v0.7 - Point Cloud Data\n"
              "VERSION 0.7\n"
              "FIELDS x y z rgb\n"
              "SIZE 4 4 4 4\n"
              "TYPE F F F U\n"
              "COUNT 1 1 1 1\n"
              "WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              "POINTS {n}\n"
              "DATA ascii\n")


def ply_text(points):
    """Mapper::exportPLY's file for MAP_POINT_DTYPE records: r = g = b = gray, coordinates in ostream's default format (%.6g)."""
    lines = [PLY_HEADER.format(n=len(points))]
    for p in points:
        g = int(p["gray"])
        lines.append("%.6g %.6g %.6g %d %d %d\n" % (p["X"][0], p["X"][1], p["X"][2], g, g, g))
    return "".join(lines)


def pcd_text(points):
    """Mapper::exportPCD's file: rgb packed as (r << 16) | (g << 8) | b."""
    lines = [PCD_HEADER.format(n=len(points))]
    for p in points:
        g = int(p["gray"])
        lines.append("%.6g %.6g %.6g %d\n" % (p["X"][0], p["X"][1], p["X"][2], (g << 16) | (g << 8) | g))
    return "".join(lines)


def _pose12(T):
    T = np.asarray(T, np.float64)
    if T.shape == (4, 4):
        T = T[:3]
    return np.ascontiguousarray(T.reshape(-1)[:12])


class HipMapper(StageHandle):
    """Binding of aria_map_t. K = (fx, fy, cx, cy); defaults are EuRoC cam0 and the reference Mapper's thresholds."""

    _prefix, _config = "map", _lib.MapConfig

    def __init__(self, K=None, min_depth=0.1, max_depth=50.0, min_parallax=1.0, max_reproj=2.0, capacity=1 << 16,
                 min_pose_inliers=10, stream=None, device=0):
        cfg = self._default_config(device, stream)
        if K is not None:
            cfg.fx, cfg.fy, cfg.cx, cfg.cy = (float(v) for v in K)
        cfg.min_depth, cfg.max_depth = min_depth, max_depth
        cfg.min_parallax_deg, cfg.max_reproj_px = min_parallax, max_reproj
        cfg.capacity = capacity
        cfg.min_pose_inliers = min_pose_inliers
        self._create(cfg)

    @property
    def K(self):
        return (self.config.fx, self.config.fy, self.config.cx, self.config.cy)

    def triangulate(self, kp1, kp2, matches, pose1, pose2, image=None, mask=None, query_is_first=True, pair_id=0):
        """One pair from host arrays; blocks and appends. kp1 = the query keypoints, kp2 = the train keypoints (frame dicts or
        KP_DTYPE arrays); pose1 / pose2: world-to-camera [R | t] (3x4, 4x4 or 12 values) of views 1 and 2; image: view 1's
        gray image (H, W) uint8. Returns the number of points added."""
        kq = kp1["keypoints"] if isinstance(kp1, dict) else kp1
        kt = kp2["keypoints"] if isinstance(kp2, dict) else kp2
        kq = np.ascontiguousarray(kq).view(KP_DTYPE).reshape(-1)
        kt = np.ascontiguousarray(kt).view(KP_DTYPE).reshape(-1)
        m = np.ascontiguousarray(matches)
        if len(m) and m.dtype != MATCH_DTYPE:
            m = m.view(MATCH_DTYPE)
        p1, p2 = _pose12(pose1), _pose12(pose2)
        img = None if image is None else np.ascontiguousarray(image, np.uint8)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mk is not None and len(mk) < len(m):
            raise ValueError("mask shorter than the match list")
        added = C.c_int(0)
        check(self._L.aria_map_triangulate(self._h, kq.ctypes.data if len(kq) else None, len(kq),
                                           kt.ctypes.data if len(kt) else None, len(kt), m.ctypes.data if len(m) else None,
                                           len(m), 1 if query_is_first else 0, p1.ctypes.data, p2.ctypes.data,
                                           None if img is None else img.ctypes.data, 0 if img is None else img.shape[1],
                                           0 if img is None else img.shape[0], 0 if img is None else img.strides[0],
                                           None if mk is None else mk.ctypes.data, pair_id, C.byref(added)),
              "aria_map_triangulate")
        return added.value

    def triangulate_batch_device(self, d_kp_query, d_nq, d_kp_train, d_nt, kp_stride, d_matches, d_nmatches, n_pairs, match_cap,
                                 d_extrinsics=None, d_pose=None, d_mask=None, d_img=None, img_stride=0, width=0, height=0,
                                 pitch=0, d_added=None, query_is_first=True, pair_base=0):
        """aria_map_triangulate_batch_device: device pointers (torch tensors or ints). Poses from d_extrinsics (24 doubles per
        pair) or, when None, d_pose (POSE_RESULT_DTYPE records). Enqueued on the handle's stream; check() synchronises and
        reports deferred errors."""
        check(self._L.aria_map_triangulate_batch_device(
            self._h, _ptr(d_kp_query), _ptr(d_nq), _ptr(d_kp_train), _ptr(d_nt), kp_stride, _ptr(d_matches), _ptr(d_nmatches),
            n_pairs, match_cap, 1 if query_is_first else 0, pair_base, _ptr(d_extrinsics), _ptr(d_pose), _ptr(d_mask),
            _ptr(d_img), img_stride, width, height, pitch, _ptr(d_added)), "aria_map_triangulate_batch_device")

    def size(self):
        n = C.c_int64(0)
        check(self._L.aria_map_size(self._h, C.byref(n)), "aria_map_size")
        return n.value

    __len__ = size

    @property
    def capacity(self):
        return self._L.aria_map_capacity(self._h)

    def points_needed(self):
        n = C.c_int64(0)
        check(self._L.aria_map_points_needed(self._h, C.byref(n)), "aria_map_points_needed")
        return n.value

    def clear(self):
        check(self._L.aria_map_clear(self._h), "aria_map_clear")

    def reserve(self, n):
        check(self._L.aria_map_reserve(self._h, int(n)), "aria_map_reserve")

    def read(self, first=0, count=None):
        """MAP_POINT_DTYPE records [first, first + count) of the map (all from `first` by default). Blocks."""
        if count is None:
            count = self.size() - first
        out = np.zeros(max(count, 1), MAP_POINT_DTYPE)
        check(self._L.aria_map_read(self._h, first, count, out.ctypes.data), "aria_map_read")
        return out[:count]

    def device_points(self):
        """Device address of the arena (size() records); valid until the next reserve, grow or filter."""
        return self._L.aria_map_device_points(self._h)

    def filter_outliers(self):
        check(self._L.aria_map_filter_outliers(self._h), "aria_map_filter_outliers")

    def filter_distance(self, max_distance=100.0):
        check(self._L.aria_map_filter_distance(self._h, float(max_distance)), "aria_map_filter_distance")

    def export_ply(self, path):
        with open(path, "w") as f:
            f.write(ply_text(self.read()))

    def export_pcd(self, path):
        with open(path, "w") as f:
            f.write(pcd_text(self.read()))
