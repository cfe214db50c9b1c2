"""Mesh of the volume on the device (include/aria_orb_hip.h, "mesh of the volume"): the records of a TSDF volume contoured
into a closed, oriented triangle mesh by marching tetrahedra on the Kuhn split of every cell. The reference has no code for
it; aria_slam_amd.mesh_ref is the definition and the device equals it byte for byte. The stage owns no volume: update()
hands it the records of a HipTsdfVolume where they lie in HBM.

As with the other stages, the handle's own stream is non-blocking: a volume filled on another stream (the volume handle's
own) must be synchronised before update(), or the mesher must be created on that stream."""
import ctypes as C

import numpy as np

from . import _lib, mesh_ref
from ._handle import StageHandle
from ._lib import MESH_TRIANGLE_DTYPE, MESH_VERTEX_DTYPE, check
from .frontend import _ptr
from .mapper import PLY_HEADER


class HipVolumeMesher(StageHandle):
    """Binding of aria_mesh_t. dims, voxel, origin and min_weight are those of the volume that is meshed."""

    _prefix, _config = "mesh", _lib.MeshConfig

    def __init__(self, dims=None, voxel=None, origin=None, min_weight=None, stream=None, device=0):
        cfg = self._default_config(device, stream)
        if dims is not None:
            cfg.nx, cfg.ny, cfg.nz = dims
        if origin is not None:
            cfg.origin[0], cfg.origin[1], cfg.origin[2] = (float(v) for v in origin)
        for name, v in (("voxel", voxel), ("min_weight", min_weight)):
            if v is not None:
                setattr(cfg, name, v)
        self._create(cfg)

    @classmethod
    def from_volume(cls, vol, **kw):
        """A mesher of the geometry (dims, voxel, origin) and min_weight of a HipTsdfVolume, on its device, already updated
        from the volume. The volume's stream is synchronised first."""
        c = vol.config
        d = dict(dims=(c.nx, c.ny, c.nz), voxel=c.voxel, origin=tuple(c.origin), min_weight=c.min_weight, device=c.device)
        d.update(kw)
        m = cls(**d)
        vol.check()
        m.update(vol)
        return m

    @property
    def ref_config(self):
        """The configuration as mesh_ref.Config."""
        c = self.config
        return mesh_ref.config(dims=(c.nx, c.ny, c.nz), voxel=c.voxel, origin=tuple(c.origin), min_weight=c.min_weight)

    def update(self, vol):
        """aria_mesh_update_from_volume_device from a HipTsdfVolume of this geometry (or the device address of its records):
        remembers the address and rebuilds the word per voxel; enqueued on this handle's stream. The object is held until
        the next update or close(), so a tensor passed here cannot be freed under the handle. Call it again after the
        volume changed."""
        if hasattr(vol, "device_voxels"):
            c, v = self.config, vol.config
            if (c.nx, c.ny, c.nz, c.voxel, tuple(c.origin)) != (v.nx, v.ny, v.nz, v.voxel, tuple(v.origin)):
                raise ValueError("the volume has another geometry (dims, voxel or origin) than the mesher")
            ptr = vol.device_voxels()
        else:
            ptr = _ptr(vol)
        check(self._L.aria_mesh_update_from_volume_device(self._h, ptr), "aria_mesh_update_from_volume_device")
        self._records = vol                                          # the handle holds their address: keep them alive

    def close(self):
        super().close()
        self._records = None

    def extract_device(self, d_vertices, vcap, d_triangles, tcap, d_counts):
        """aria_mesh_extract_device: vcap MESH_VERTEX_DTYPE records at d_vertices, tcap MESH_TRIANGLE_DTYPE records at
        d_triangles (either None with capacity 0), the two int64 totals at d_counts. Enqueued; check() synchronises and
        reports a total above its capacity."""
        check(self._L.aria_mesh_extract_device(self._h, _ptr(d_vertices), vcap, _ptr(d_triangles), tcap, _ptr(d_counts)),
              "aria_mesh_extract_device")

    def count(self):
        """(vertices, triangles) the mesh of the last update holds; blocks."""
        n = (C.c_int64 * 2)()
        rc = self._L.aria_mesh_extract(self._h, None, 0, None, 0, n)
        if rc not in (_lib.ARIA_OK, _lib.ARIA_E_OUTPUT_TOO_SMALL):
            check(rc, "aria_mesh_extract")
        return n[0], n[1]

    def extract(self, vcap=None, tcap=None):
        """(vertices, triangles) as MESH_VERTEX_DTYPE and MESH_TRIANGLE_DTYPE records in canonical order; blocks. With a
        capacity below a total the first records come back together with the totals: (vertices, triangles, (nv, nt))."""
        nv, nt = self.count() if vcap is None or tcap is None else (vcap, tcap)
        nv, nt = (nv if vcap is None else vcap), (nt if tcap is None else tcap)
        verts, tris = np.zeros(nv, MESH_VERTEX_DTYPE), np.zeros(nt, MESH_TRIANGLE_DTYPE)
        n = (C.c_int64 * 2)()
        rc = self._L.aria_mesh_extract(self._h, verts.ctypes.data if nv else None, nv, tris.ctypes.data if nt else None, nt, n)
        if vcap is None and tcap is None:
            check(rc, "aria_mesh_extract")
            return verts, tris
        if rc != _lib.ARIA_E_OUTPUT_TOO_SMALL:
            check(rc, "aria_mesh_extract")
        return verts[:min(nv, n[0])], tris[:min(nt, n[1])], (n[0], n[1])

    def export_ply(self, path):
        """The mesh as an ASCII PLY: the header and vertex format HipMapper.export_ply writes (r = g = b = gray) plus the
        faces as `property list uchar int vertex_indices`."""
        with open(path, "w") as f:
            f.write(ply_text(*self.extract()))


def ply_text(vertices, triangles):
    """The ASCII PLY of a mesh: mapper.PLY_HEADER's vertex block, then `element face`."""
    head = PLY_HEADER.format(n=len(vertices)).replace(
        "end_header\n", "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(triangles))
    lines = [head]
    for p in vertices:
        g = int(p["gray"])
        lines.append("%.6g %.6g %.6g %d %d %d\n" % (p["X"][0], p["X"][1], p["X"][2], g, g, g))
    for t in np.asarray(triangles)["v"].reshape(-1, 3):
        lines.append("3 %d %d %d\n" % (t[0], t[1], t[2]))
    return "".join(lines)


def read_ply(path):
    """(X float64 [n, 3], gray uint8 [n], faces int64 [m, 3]) of a PLY written by export_ply or euroc_frontend --mesh."""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    nv = nf = 0
    for ln in lines[:end]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        if w[:2] == ["element", "face"]:
            nf = int(w[2])
    body = lines[end + 1:]
    v = np.array([ln.split() for ln in body[:nv]], np.float64).reshape(nv, 6)
    f_ = np.array([ln.split() for ln in body[nv:nv + nf]], np.int64).reshape(nf, 4)
    assert (f_[:, 0] == 3).all()
    return v[:, :3], v[:, 3].astype(np.uint8), f_[:, 1:]


def scratch_bytes(nx, ny, nz):
    return _lib.load_library().aria_mesh_scratch_bytes(nx, ny, nz)


def algorithmic_bytes(nx, ny, nz, n_vertices, n_triangles):
    return _lib.load_library().aria_mesh_algorithmic_bytes(nx, ny, nz, n_vertices, n_triangles)
