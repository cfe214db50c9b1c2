"""Shared inputs of the mesh tests (test_mesh_host.py, test_mesh_kernel_emulation.py, test_gpu_mesh.py): record volumes of
every kind the device tests run, the restatement's results on them (aria_slam_amd/mesh_ref.py), computed once per process and
handed out read-only, and the host build of the kernel file's per-voxel and per-cell functions."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import tsdf_cases as TC
from aria_slam_amd import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
GUARD = 0x5A
MIN_WEIGHT = 3
f32 = np.float32


def config(dims, **kw):
    d = dict(dims=dims, voxel=0.1, origin=(-0.4, 0.3, 1.0), min_weight=MIN_WEIGHT)
    d.update(kw)
    return M.config(**d)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_records(dims, seed=0, unseen=0.0, special=True):
    """Records [nz, ny, nx] with tsdf uniform in [-1, 1]; with `special` a tenth of them are exact zeros, -0.0f and the values
    one ulp either side of zero, and the weights are min_weight and 65535; a share `unseen` has weight min_weight - 1."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    vol = np.zeros((nz, ny, nx), M.VOXEL_DTYPE)
    t = rng.uniform(-1, 1, vol.shape).astype(f32)
    if special:
        tiny = np.nextafter(f32(0), f32(1))
        kinds = np.array([0.0, -0.0, tiny, -tiny], f32)
        pick = rng.random(vol.shape) < 0.1
        t[pick] = kinds[rng.integers(0, 4, int(pick.sum()))]
    vol["tsdf"] = t
    vol["weight"] = np.where(rng.random(vol.shape) < 0.5, MIN_WEIGHT, 65535)
    if unseen:
        vol["weight"][rng.random(vol.shape) < unseen] = MIN_WEIGHT - 1
    vol["gray"] = rng.integers(0, 256, vol.shape)
    return _ro(vol)


@functools.lru_cache(maxsize=None)
def sign_records(dims, seed=0):
    """Random signs, all seen, with an outside border: the mesh is closed."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    vol = np.zeros((nz, ny, nx), M.VOXEL_DTYPE)
    vol["tsdf"] = 1.0
    vol["tsdf"][1:-1, 1:-1, 1:-1] = np.where(rng.random((nz - 2, ny - 2, nx - 2)) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 1, (nz - 2, ny - 2, nx - 2))
    vol["weight"] = MIN_WEIGHT
    return _ro(vol)


@functools.lru_cache(maxsize=None)
def shell_records(dims=(72, 64, 64)):
    """A sphere that nearly fills the volume, seen only in a thin shell around its surface: few vertices in many chunks, the
    last of them near the end of the volume."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz, dtype=f32), np.arange(ny, dtype=f32), np.arange(nx, dtype=f32), indexing="ij")
    d = np.sqrt((x - f32(0.49 * nx)) ** 2 + (y - f32(0.47 * ny)) ** 2 + (z - f32(0.527 * nz)) ** 2) - f32(0.43 * min(dims))
    vol = np.zeros((nz, ny, nx), M.VOXEL_DTYPE)
    vol["tsdf"] = np.clip(d / f32(3), -1, 1)
    vol["weight"] = np.where(np.abs(d) < 2.5, MIN_WEIGHT + 2, 0)
    vol["gray"] = (x + 2 * y + 3 * z).astype(np.int64) % 256
    return _ro(vol)


def sphere_records():
    """The known answer: 20^3 voxels, tsdf = distance to a sphere, every voxel seen (dims outside the configuration's range:
    for the restatement alone)."""
    z, y, x = np.meshgrid(*(np.arange(20, dtype=f32),) * 3, indexing="ij")
    vol = np.zeros((20, 20, 20), M.VOXEL_DTYPE)
    vol["tsdf"] = np.sqrt((x - f32(9.3)) ** 2 + (y - f32(10.1)) ** 2 + (z - f32(9.7)) ** 2) - f32(6.2)
    vol["weight"] = 1
    return vol, M.Config((20, 20, 20), f32(1), (f32(0), f32(0), f32(0)), 1)


def scene():
    """(cfg, records) of the three-pose scene of tests/tsdf_cases.py at 32 x 24 x 16, as the fusion's restatement leaves it."""
    tcfg, vol, _ = TC.ref_scene()
    return M.config(dims=tcfg.dims, voxel=tcfg.voxel, origin=tcfg.origin, min_weight=tcfg.min_weight), vol


_cache = {}


def ref(name, vol, cfg):
    """(vertices, triangles, totals) of the restatement under `name`, computed once per process; read-only."""
    if name not in _cache:
        v, t, n = M.extract(vol, cfg)
        _cache[name] = (_ro(v), _ro(t), n)
    return _cache[name]


def random_case(dims, unseen):
    """(cfg, records, the restatement's result) of the random records every mesh test shares for these dims."""
    cfg, vol = config(dims), random_records(dims, dims[0] + int(round(unseen * 100)), unseen)
    return cfg, vol, ref("random_%r_%r" % (dims, unseen), vol, cfg)


@functools.lru_cache(maxsize=None)
def emu():
    """The per-voxel and per-cell functions of tsdf_mesh.hip compiled for the host between the two shim files."""
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    src = open(os.path.join(csrc, "tsdf_mesh.hip")).read()
    body = src[src.index("\nnamespace {"):src.index("\n// ---- kernels")]
    for name in ("mesh_voxel", "mesh_vertex", "mesh_vertex_number", "mesh_cell_triangles", "mesh_count_errors", "MESH_TABLE"):
        assert name in body, name
    assert "asm" not in body and "__shared__" not in body and "__syncthreads" not in body and "atomic" not in body
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("mesh_kernel_emu_head.inc", "mesh_kernel_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "mesh_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "mesh_emu.cpp"), os.path.join(out_dir, "libmesh_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + parts[1])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "-o", so, cpp])
    L = C.CDLL(so)
    p, i64 = C.c_void_p, C.c_int64
    L.emu_mesh_table.restype = C.c_uint64
    L.emu_mesh_table.argtypes = [C.c_int, C.c_int]
    L.emu_mesh_scan.argtypes = [p, p, i64, i64, i64, p, p, p]
    L.emu_mesh_extract.argtypes = [p, p, p, p, p, p, p, p, p, i64, p, i64, p]
    return L


def emu_extract(vol, cfg, vcap=None, tcap=None, fill=GUARD):
    """The host build over records: (vertices, triangles, totals, error bits). With capacities the arrays keep their full
    length (vcap, tcap), pre-filled with `fill` bytes."""
    L = emu()
    nx, ny, nz = cfg.dims
    n_vox = nx * ny * nz
    rec = np.ascontiguousarray(vol)
    dims = np.array([nx, ny, nz, cfg.min_weight], np.int32)
    geom = np.array([cfg.voxel, *cfg.origin], f32)
    words = np.zeros(n_vox, np.uint32)
    vc, tc = np.zeros(n_vox // 256, np.int32), np.zeros(n_vox // 256, np.int32)
    vo, to = np.zeros(n_vox // 256, np.int64), np.zeros(n_vox // 256, np.int64)
    totals = np.zeros(2, np.int64)
    if vcap is None or tcap is None:
        bits = L.emu_mesh_extract(dims.ctypes.data, geom.ctypes.data, rec.ctypes.data, words.ctypes.data, vc.ctypes.data, tc.ctypes.data,
                                  vo.ctypes.data, to.ctypes.data, None, 0, None, 0, totals.ctypes.data)
        assert bits in (0, 1)
        vcap, tcap = (int(totals[0]) if vcap is None else vcap), (int(totals[1]) if tcap is None else tcap)
    verts = np.frombuffer(bytes([fill]) * (16 * vcap), M.VERTEX_DTYPE).copy()
    tris = np.frombuffer(bytes([fill]) * (12 * tcap), M.TRIANGLE_DTYPE).copy()
    bits = L.emu_mesh_extract(dims.ctypes.data, geom.ctypes.data, rec.ctypes.data, words.ctypes.data, vc.ctypes.data, tc.ctypes.data,
                              vo.ctypes.data, to.ctypes.data, verts.ctypes.data if vcap else None, vcap, tris.ctypes.data if tcap else None,
                              tcap, totals.ctypes.data)
    return verts, tris, (int(totals[0]), int(totals[1])), bits
