"""Path planning on the device (include/aria_orb_hip.h, "path planning"): a 2-D traversability grid collapsed out of a
height band of a HipTsdfVolume, an exact clearance field and an integer cost map, exact cost-to-go fields for a batch of
goals and paths traced for a batch of queries. The reference has no code for it; aria_slam_amd.nav_ref is the definition
and the device equals it bit for bit.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on another stream (torch's
default stream, another handle's) must be synchronised before a *_device call, or the handle must be created on that
stream. Arrays over the grid are [nv, nu]; cell (u, v) has the linear index v*nu + u."""
import numpy as np

from . import _lib, nav_ref
from ._handle import StageHandle
from ._lib import NAV_RECORD_DTYPE, check
from .frontend import _ptr

_FIELDS = ("up_axis", "min_weight", "occ_tsdf", "occ_count", "free_count", "clear_radius", "block_d2", "soft_d2", "penalty",
           "unknown_penalty", "allow_unknown", "max_goals", "voxel")


class HipPathPlanner(StageHandle):
    """Binding of aria_nav_t. dims = (nx, ny, nz) of the volume; band = (band0, band1) on up_axis, by default
    [n/2 - 8, n/2 + 16) cut to the axis. The default band and radii are assumptions nobody has tuned on a recording."""

    _prefix, _config = "nav", _lib.NavConfig

    def __init__(self, dims=None, up_axis=None, band=None, min_weight=None, occ_tsdf=None, occ_count=None, free_count=None,
                 clear_radius=None, block_d2=None, soft_d2=None, penalty=None, unknown_penalty=None, allow_unknown=None,
                 max_goals=None, voxel=None, origin=None, stream=None, device=0):
        cfg = self._default_config(device, stream)
        if dims is not None:
            cfg.nx, cfg.ny, cfg.nz = dims
        if origin is not None:
            cfg.origin[0], cfg.origin[1], cfg.origin[2] = (float(v) for v in origin)
        given = dict(up_axis=up_axis, min_weight=min_weight, occ_tsdf=occ_tsdf, occ_count=occ_count, free_count=free_count,
                     clear_radius=clear_radius, block_d2=block_d2, soft_d2=soft_d2, penalty=penalty, unknown_penalty=unknown_penalty,
                     allow_unknown=allow_unknown, max_goals=max_goals, voxel=voxel)
        for name in _FIELDS:
            if given[name] is not None:
                setattr(cfg, name, given[name])
        if band is not None:
            cfg.band0, cfg.band1 = band
        elif cfg.up_axis in (0, 1, 2):
            cfg.band0, cfg.band1 = nav_ref.default_band((cfg.nx, cfg.ny, cfg.nz)[cfg.up_axis])
        self._create(cfg)

    @classmethod
    def from_volume(cls, vol, **kw):
        """A planner of the geometry (dims, voxel, origin) of a HipTsdfVolume, on its device; min_weight is the volume's
        unless given."""
        c = vol.config
        d = dict(dims=(c.nx, c.ny, c.nz), voxel=c.voxel, origin=tuple(c.origin), min_weight=c.min_weight, device=c.device)
        d.update(kw)
        return cls(**d)

    @property
    def ref_config(self):
        """The configuration as nav_ref.Config."""
        c = self.config
        d = {name: getattr(c, name) for name in _FIELDS}
        return nav_ref.config(dims=(c.nx, c.ny, c.nz), band=(c.band0, c.band1), origin=tuple(c.origin), **d)

    @property
    def shape(self):
        """(nv, nu): the shape of the arrays over the grid."""
        c = self.config
        dims = (c.nx, c.ny, c.nz)
        U, V = nav_ref.plane_axes(c.up_axis)
        return dims[V], dims[U]

    def update(self, vol):
        """Rules 2-4 from a HipTsdfVolume of this geometry (or the device address of its records); enqueued on this handle's
        stream: the volume's own stream must have been synchronised, or be this one."""
        ptr = vol.device_voxels() if hasattr(vol, "device_voxels") else _ptr(vol)
        check(self._L.aria_nav_update_from_volume_device(self._h, ptr), "aria_nav_update_from_volume_device")

    def set_cells(self, cells):
        """Rules 3-4 on given cells, uint8 [nv, nu] of 0 FREE, 1 OCCUPIED, 2 UNKNOWN; blocks."""
        a = np.ascontiguousarray(cells, np.uint8)
        if a.shape != self.shape:
            raise ValueError("cells are uint8 [nv, nu] = %r" % (self.shape,))
        check(self._L.aria_nav_set_cells(self._h, a.ctypes.data), "aria_nav_set_cells")

    def set_cells_device(self, d_cells):
        """aria_nav_set_cells_device: nu*nv bytes in HBM; enqueued. A value above 2 defers ARIA_E_INVALID and keeps the old
        cells."""
        check(self._L.aria_nav_set_cells_device(self._h, _ptr(d_cells)), "aria_nav_set_cells_device")

    def _read(self, fn, dtype):
        out = np.zeros(self.shape, dtype)
        check(fn(self._h, out.ctypes.data), fn.__name__)
        return out

    def cells(self):
        return self._read(self._L.aria_nav_read_cells, np.uint8)

    def clearance(self):
        return self._read(self._L.aria_nav_read_clearance, np.uint16)

    def costs(self):
        return self._read(self._L.aria_nav_read_costs, np.uint16)

    def solve_device(self, d_goals, n_goals):
        """aria_nav_solve_device: 2*n_goals int32 (u, v) in HBM; enqueued."""
        check(self._L.aria_nav_solve_device(self._h, _ptr(d_goals), n_goals), "aria_nav_solve_device")

    def trace_device(self, d_queries, n_queries, d_records, d_paths, path_cap):
        """aria_nav_trace_device: 3*n_queries int32 (su, sv, goal_index) in HBM, NAV_RECORD_DTYPE records and
        n_queries*path_cap int32 path cells out; enqueued."""
        check(self._L.aria_nav_trace_device(self._h, _ptr(d_queries), n_queries, _ptr(d_records), _ptr(d_paths), path_cap),
              "aria_nav_trace_device")

    def plan(self, goals, queries, path_cap, paths=None):
        """Solve and trace from host arrays; blocks. goals [G, 2] (u, v), queries [Q, 3] (su, sv, goal_index). Returns
        (records [Q], paths [Q, path_cap], truncated): path entries beyond a query's cells keep the bytes of `paths` (zero
        without one); truncated = some query has status TRUNCATED."""
        g = np.ascontiguousarray(np.asarray(goals, np.int32).reshape(-1, 2))
        q = np.ascontiguousarray(np.asarray(queries, np.int32).reshape(-1, 3))
        rec = np.zeros(len(q), NAV_RECORD_DTYPE)
        out = np.zeros((len(q), path_cap), np.int32) if paths is None else np.ascontiguousarray(paths, np.int32).reshape(len(q), path_cap)
        rc = self._L.aria_nav_plan(self._h, g.ctypes.data if len(g) else None, len(g), q.ctypes.data if len(q) else None, len(q),
                                   rec.ctypes.data if len(q) else None, out.ctypes.data if out.size else None, path_cap)
        if rc != _lib.ARIA_E_OUTPUT_TOO_SMALL:
            check(rc, "aria_nav_plan")
        return rec, out, rc == _lib.ARIA_E_OUTPUT_TOO_SMALL

    def field(self, g):
        """The field of goal g of the last solve, int32 [nv, nu]; blocks."""
        out = np.zeros(self.shape, np.int32)
        check(self._L.aria_nav_read_field(self._h, g, out.ctypes.data), "aria_nav_read_field")
        return out

    def rounds(self, n_goals):
        """The relaxation rounds each of the first n_goals goals of the last solve took; blocks."""
        out = np.zeros(n_goals, np.int32)
        check(self._L.aria_nav_read_rounds(self._h, out.ctypes.data, n_goals), "aria_nav_read_rounds")
        return out

    def device_fields(self):
        """The device address of the field buffer (aria_nav_device_fields)."""
        return self._L.aria_nav_device_fields(self._h)

    def cell_of(self, X):
        """World points [n, 3] to cells [n, 2] (u, v), on the host: floor((x - origin) / voxel) in fp32 on the plane axes."""
        return nav_ref.cell_of(X, self.ref_config)

    def centre_of(self, cells):
        """Cells [n, 2] to world points [n, 3], on the host: the voxel centre on the plane axes, the middle of the band on
        up_axis."""
        return nav_ref.centre_of(cells, self.ref_config)


def field_bytes(nu, nv, max_goals):
    return _lib.load_library().aria_nav_field_bytes(nu, nv, max_goals)
