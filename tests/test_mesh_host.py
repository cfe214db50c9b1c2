"""Mesh of the volume (include/aria_orb_hip.h, "mesh of the volume"): the parts that need no GPU -- exports, the layouts,
defaults and validation, the NumPy restatement (aria_slam_amd/mesh_ref.py, which is the definition) against a plain per-cell
loop, its table, its known answer and the closure properties of rule 7, the axis vertices against the fusion's surface
points, the accuracy of the diagonal-edge vertices on the analytic scene, the capacity cut, the scan's 2^32 comparison and the
kernels' listing."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_kernel_stats as S   # noqa: E402
import mesh_cases as MC   # noqa: E402
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import mesh_ref as M   # noqa: E402
from aria_slam_amd import tsdf_ref   # noqa: E402

MESH_SYMBOLS = ["aria_mesh_default_config", "aria_mesh_create", "aria_mesh_destroy", "aria_mesh_stream", "aria_mesh_check",
                "aria_mesh_update_from_volume_device", "aria_mesh_extract_device", "aria_mesh_extract", "aria_mesh_scratch_bytes",
                "aria_mesh_algorithmic_bytes"]
KERNELS = ("k_mesh_count", "k_mesh_scan", "k_mesh_emit")
f32 = np.float32


def test_mesh_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in MESH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipVolumeMesher" in aria.__all__
    for word in ("256-case", "vertex normals", "welding or decimation", "colour beyond gray", "meshing a sub-box", "bricks that changed"):
        assert word in header, "out of scope: %s" % word


def test_mesh_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    assert C.sizeof(_lib.MeshConfig) == 48
    assert _lib.MESH_VERTEX_DTYPE.itemsize == 16 and _lib.MESH_VERTEX_DTYPE == M.VERTEX_DTYPE
    assert _lib.MESH_TRIANGLE_DTYPE.itemsize == 12 and _lib.MESH_TRIANGLE_DTYPE == M.TRIANGLE_DTYPE
    assert M.VOXEL_DTYPE == tsdf_ref.VOXEL_DTYPE
    cfg = _lib.MeshConfig()
    L.aria_mesh_default_config(C.byref(cfg))
    assert cfg.struct_size == 48 and not cfg.stream
    assert (cfg.nx, cfg.ny, cfg.nz, cfg.min_weight, cfg.voxel) == (256, 256, 128, 2, f32(0.05))
    d = M.config()
    assert d.dims == (256, 256, 128) and d.voxel == cfg.voxel and tuple(d.origin) == tuple(f32(v) for v in cfg.origin) and d.min_weight == 2
    n = 256 * 256 * 128
    assert L.aria_mesh_scratch_bytes(256, 256, 128) == 4 * n + 24 * (n // 256) == M.scratch_bytes(256, 256, 128)
    assert L.aria_mesh_scratch_bytes(12, 8, 8) == -1 and L.aria_mesh_scratch_bytes(8, 8, 1032) == -1
    assert L.aria_mesh_algorithmic_bytes(256, 256, 128, 1000, 2000) == 16 * n + 16 * 1000 + 12 * 2000 == M.algorithmic_bytes(256, 256, 128, 1000, 2000)
    assert L.aria_mesh_algorithmic_bytes(256, 256, 128, -1, 0) == -1 and L.aria_mesh_algorithmic_bytes(256, 256, 4, 0, 0) == -1


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("nx", 12), ("ny", 0), ("nz", 1032), ("nz", 4), ("voxel", 0.0),
                                         ("voxel", float("nan")), ("voxel", float("inf")), ("min_weight", 0), ("min_weight", 65536)])
def test_mesh_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched, and the restatement refuses the same."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.MeshConfig()
    L.aria_mesh_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_mesh_create(C.byref(cfg), C.byref(h)) == -1        # ARIA_E_INVALID
    assert not h.value
    assert L.aria_mesh_create(None, C.byref(h)) == -1 and L.aria_mesh_create(C.byref(cfg), None) == -1
    if field in ("nx", "ny", "nz"):
        dims = {"nx": 256, "ny": 256, "nz": 128}
        dims[field] = value
        with pytest.raises(ValueError):
            M.config(dims=(dims["nx"], dims["ny"], dims["nz"]))
    elif field != "struct_size":
        with pytest.raises(ValueError):
            M.config(**{field: value})
    cfg = _lib.MeshConfig()
    L.aria_mesh_default_config(C.byref(cfg))
    cfg.origin[1] = float("nan")
    assert L.aria_mesh_create(C.byref(cfg), C.byref(h)) == -1


def test_mesh_calls_refuse_null_handles(aria):
    L = aria.load_library()
    n = (C.c_int64 * 2)()
    assert L.aria_mesh_update_from_volume_device(None, None) == -1
    assert L.aria_mesh_extract_device(None, None, 0, None, 0, n) == -1
    assert L.aria_mesh_extract(None, None, 0, None, 0, n) == -1
    assert L.aria_mesh_check(None) == -1 and L.aria_mesh_stream(None) is None
    L.aria_mesh_destroy(None)
    L.aria_mesh_default_config(None)


def test_no_gpu_means_mesh_create_fails_loudly(aria):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(aria.AriaError) as e:
        aria.HipVolumeMesher(dims=(8, 8, 8))
    assert e.value.status == -2                                      # ARIA_E_NO_DEVICE: there is no CPU fallback


# ---- the restatement against a plain loop ----------------------------------------------------------------------------------
def _loop_mesh(vol, cfg):
    """Rules 2-5 voxel by voxel and cell by cell, with no table: every tetrahedron's polygon is built and oriented on the spot
    from the corner coordinates."""
    nx, ny, nz = cfg.dims
    bits = lambda q: (q & 1, (q >> 1) & 1, (q >> 2) & 1)   # noqa: E731
    seen = lambda r: r["weight"] >= cfg.min_weight   # noqa: E731
    number, verts = {}, []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                a = vol[k, j, i]
                for d in range(1, 8):
                    dx, dy, dz = bits(d)
                    if i + dx >= nx or j + dy >= ny or k + dz >= nz:
                        continue
                    b = vol[k + dz, j + dy, i + dx]
                    if not (seen(a) and seen(b)) or (a["tsdf"] < 0) == (b["tsdf"] < 0):
                        continue
                    alpha = a["tsdf"] / (a["tsdf"] - b["tsdf"])
                    step = alpha * cfg.voxel
                    X = [cfg.origin[n] + (f32(v) + f32(0.5)) * cfg.voxel for n, v in enumerate((i, j, k))]
                    for n in range(3):
                        if bits(d)[n]:
                            X[n] = X[n] + step
                    v = np.zeros((), M.VERTEX_DTYPE)
                    v["X"], v["dir"] = X, d
                    v["gray"] = a["gray"] if alpha < f32(0.5) else b["gray"]
                    v["weight"] = min(a["weight"], b["weight"])
                    number[(i, j, k, d)] = len(verts)
                    verts.append(v)
    tris = []
    perms = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corner = [vol[k + bz, j + by, i + bx] for bx, by, bz in map(bits, range(8))]
                if not all(seen(c) for c in corner):
                    continue
                for pi in perms:
                    tet = (0, 1 << pi[0], (1 << pi[0]) + (1 << pi[1]), 7)
                    ins = [t for t in range(4) if corner[tet[t]]["tsdf"] < 0]
                    out = [t for t in range(4) if t not in ins]
                    if len(ins) in (0, 4):
                        continue
                    if len(ins) == 1:
                        poly = [(ins[0], o) for o in out]
                    elif len(ins) == 3:
                        poly = [(n, out[0]) for n in ins]
                    else:
                        poly = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
                    xyz = [np.array(bits(q), float) for q in tet]
                    mid = [(xyz[s] + xyz[t]) / 2 for s, t in poly]
                    want = np.mean([xyz[t] for t in out], axis=0) - np.mean([xyz[t] for t in ins], axis=0)
                    split = [(0, 1, 2)] if len(poly) == 3 else [(0, 1, 2), (0, 2, 3)]
                    if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), want) < 0:
                        split = [(t[0], t[2], t[1]) for t in split]
                    for t in split:
                        tri = []
                        for e in t:
                            lo, hi = sorted((tet[poly[e][0]], tet[poly[e][1]]))
                            bx, by, bz = bits(lo)
                            tri.append(number[(i + bx, j + by, k + bz, hi - lo)])
                        tris.append(tri)
    out = np.zeros(len(tris), M.TRIANGLE_DTYPE)
    out["v"] = np.array(tris, np.int64).reshape(-1, 3)
    return np.array(verts, M.VERTEX_DTYPE), out


@pytest.mark.parametrize("unseen", [0.0, 0.15])
def test_ref_equals_a_plain_per_cell_loop(unseen):
    cfg, vol, (want_v, want_t, (nv, nt)) = MC.random_case((8, 8, 8), unseen)
    got_v, got_t = _loop_mesh(vol, cfg)
    assert nv == len(want_v) > 200 and nt == len(want_t) > 100
    assert got_v.tobytes() == want_v.tobytes() and got_t.tobytes() == want_t.tobytes()


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_table_follows_the_orientation_rule_and_the_counts():
    assert M.TRIANGLE_COUNTS == (0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0)
    xyz = lambda q: np.array([q & 1, (q >> 1) & 1, (q >> 2) & 1], float)   # noqa: E731
    assert M.TET_CORNERS == ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
    for p, corners in enumerate(M.TET_CORNERS):
        for mask in range(16):
            tris = M.TABLE[p][mask]
            assert len(tris) == M.TRIANGLE_COUNTS[mask]
            ins = [c for t, c in enumerate(corners) if mask >> t & 1]
            out = [c for c in corners if c not in ins]
            cut = {(lo, hi - lo) for lo in corners for hi in corners if lo < hi and (lo in ins) != (hi in ins)}
            assert {e for tri in tris for e in tri} == cut           # every cut edge of the tetrahedron, and no other
            for tri in tris:
                assert all(1 <= d <= 7 and 0 <= lo <= 6 and lo & d == 0 for lo, d in tri)
                m = [xyz(lo) + xyz(d) / 2 for lo, d in tri]
                n = np.cross(m[1] - m[0], m[2] - m[0])
                assert np.dot(n, np.mean([xyz(c) for c in out], axis=0) - np.mean([xyz(c) for c in ins], axis=0)) > 0, (p, mask)


def test_hip_constants_equal_the_derived_table():
    """The constants of tsdf_mesh_table.inc, as text and as the host build of the kernel file reads them."""
    text = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "tsdf_mesh_table.inc")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("//"))
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)ull", code)]
    assert words == M.table_words() and len(words) == 96
    assert code.strip("\n") == M.table_text().strip("\n")
    L = MC.emu()
    assert [L.emu_mesh_table(p, m) for p in range(6) for m in range(16)] == M.table_words()
    assert L.emu_mesh_block() == 256
    for p in range(6):
        for m in range(16):
            w = M.table_words()[16 * p + m]
            tris = tuple(tuple(((w >> (4 + 6 * (3 * t + c)) & 63) >> 3, (w >> (4 + 6 * (3 * t + c))) & 7) for c in range(3)) for t in range(w & 3))
            assert tris == M.TABLE[p][m]


# ---- known answers and the properties of rule 7 ----------------------------------------------------------------------------
def _euler(nv_used, tri):
    e = M.directed_edges(tri)
    return nv_used - len(np.unique(np.sort(e, axis=1), axis=0)) + len(tri)


def test_ref_known_answer_sphere():
    """20^3 voxels, tsdf = sqrt((x-9.3)^2 + (y-10.1)^2 + (z-9.7)^2) - 6.2 in fp32, every voxel seen: 2168 vertices and 4332
    triangles, every directed edge met by its reverse exactly once, V - E + F = 2."""
    vol, cfg = MC.sphere_records()
    v, t, (nv, nt) = M.extract(vol, cfg)
    dup, unmatched = M.edge_report(t["v"])
    print("vertices %d triangles %d duplicated %d unmatched %d" % (nv, nt, dup, len(unmatched)))
    assert (nv, nt) == (2168, 4332) and dup == 0 and len(unmatched) == 0
    assert len(np.unique(t["v"])) == nv and _euler(nv, t["v"]) == 2
    centre = np.array([9.3, 10.1, 9.7]) + 0.5                        # voxel i has its centre at i + 0.5
    r = np.linalg.norm(v["X"].astype(np.float64) - centre, axis=1)
    # linear interpolation of a distance field along an edge of length L <= sqrt(3): at most L^2 / 8 times its second
    # derivative, which is at most 1 / (distance to the centre) <= 1 / (6.2 - L / 2)
    assert np.abs(r - 6.2).max() <= 3.0 / 8.0 / (6.2 - np.sqrt(3.0) / 2)
    # the orientation: normals point to the outside (growing tsdf)
    X = v["X"].astype(np.float64)
    a, b, c = (X[t["v"][:, n]] for n in range(3))
    nrm = np.cross(b - a, c - a)
    assert (np.einsum("ij,ij->i", nrm, (a + b + c) / 3 - centre) > 0).all()


@pytest.mark.parametrize("dims,seed", [((8, 8, 8), 1), ((16, 8, 24), 2)])
def test_ref_random_signs_with_an_outside_border_are_closed(dims, seed):
    vol = MC.sign_records(dims, seed)
    _, t, (nv, nt) = M.extract(vol, MC.config(dims))
    dup, unmatched = M.edge_report(t["v"])
    assert nt > 500 and dup == 0 and len(unmatched) == 0


@pytest.mark.parametrize("dims,seed", [((8, 8, 8), 3), ((16, 8, 24), 4)])
def test_ref_unseen_voxels_open_the_mesh_only_at_non_live_neighbours(dims, seed):
    """With unseen voxels no directed edge appears twice, and every directed edge whose reverse is missing lies in a face of
    its cell across which the neighbouring cell is not live (or does not exist)."""
    cfg = MC.config(dims)
    vol = MC.random_records(dims, seed, unseen=0.1)
    v, t, _ = M.extract(vol, cfg)
    dup, unmatched = M.edge_report(t["v"])
    assert dup == 0 and len(unmatched) > 50
    nx, ny, nz = dims
    owner, cell = M.owners(vol, cfg)
    live = M.live_cells(vol, cfg)
    where = {}
    for n, tri in enumerate(t["v"].astype(np.int64)):
        for e in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            where[e] = n

    def ends(vertex):
        lin, d = int(owner[vertex]), int(v["dir"][vertex])
        p0 = np.array([lin % nx, lin // nx % ny, lin // (nx * ny)])
        return p0, p0 + np.array([d & 1, (d >> 1) & 1, (d >> 2) & 1])

    def is_live(c):
        return all(0 <= c[a] < dims[a] - 1 for a in range(3)) and bool(live[c[2], c[1], c[0]])

    for e in map(tuple, unmatched):
        lin = int(cell[where[e]])
        c = np.array([lin % nx, lin // nx % ny, lin // (nx * ny)])
        assert is_live(c)
        pts = [p for vertex in e for p in ends(vertex)]
        faces = [(a, s) for a in range(3) for s in (0, 1) if all(p[a] == c[a] + s for p in pts)]
        assert faces, "an unmatched edge in the interior of its cell"
        step = lambda a, s: c + (2 * s - 1) * np.eye(3, dtype=int)[a]   # noqa: E731
        assert any(not is_live(step(a, s)) for a, s in faces), (e, c)


def test_ref_exact_zeros_keep_the_topology():
    """An exact zero is outside and gives alpha = 0 towards its inside neighbours (alpha = 1 from them): every vertex on an
    edge of the zero voxel coincides with its centre, the triangles between them have no area, and the mesh stays closed.
    -0.0f is outside too."""
    cfg = M.config(dims=(8, 8, 8), voxel=1.0, origin=(0, 0, 0), min_weight=1)
    vol = np.zeros((8, 8, 8), M.VOXEL_DTYPE)
    vol["weight"] = 1
    vol["tsdf"] = 0.5
    vol["tsdf"][0, 0, 0] = 0.0
    vol["tsdf"][0, 0, 1] = -0.0
    assert M.extract(vol, cfg)[2] == (0, 0)
    vol["tsdf"][2:5, 2:5, 2:5] = -0.5
    base_v, base_t, _ = M.extract(vol, cfg)
    vol["tsdf"][3, 3, 3] = 0.0                                       # a zero surrounded by inside voxels: a bubble of no volume
    v, t, (nv, nt) = M.extract(vol, cfg)
    dup, unmatched = M.edge_report(t["v"])
    assert dup == 0 and len(unmatched) == 0 and nv > len(base_v) and nt > len(base_t)
    at_centre = (v["X"] == f32(3.5)).all(axis=1)
    assert at_centre.sum() == 14                                     # one per edge of the Kuhn grid at a voxel: 6 + 6 + 2
    X = v["X"].astype(np.float64)
    a, b, c = (X[t["v"][:, n]] for n in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    at = at_centre[t["v"]].sum(axis=1)                               # the bubble's 24 triangles, all three vertices at the centre
    assert ((area == 0) == (at == 3)).all() and (at == 3).sum() == 24 == nt - len(base_t) and set(at) == {0, 3}
    # two components now: the block's surface and the bubble, each a sphere
    assert _euler(nv, t["v"]) == 4


def test_ref_axis_vertices_are_the_fusion_surface_points():
    """Vertices with dir in {1, 2, 4}, in order, are tsdf_ref.extract's points bitwise (X, gray, weight), axis = log2(dir)."""
    cfg, vol = MC.scene()
    tcfg, _, pts = TC.ref_scene()
    v = MC.ref("scene", vol, cfg)[0]
    axis = v[np.isin(v["dir"], (1, 2, 4))]
    assert len(axis) == len(pts) > 400 and len(v) > 2 * len(pts)
    assert axis["X"].tobytes() == pts["X"].tobytes() and (axis["gray"] == pts["gray"]).all() and (axis["weight"] == pts["weight"]).all()
    assert (axis["dir"] == 1 << pts["axis"]).all()


def test_ref_capacity_cut():
    cfg, vol = MC.scene()
    want_v, want_t, (nv, nt) = MC.ref("scene", vol, cfg)
    for vcap, tcap in ((0, 0), (1, 2), (nv // 2, nt), (nv, nt // 2), (nv + 7, nt + 7)):
        v, t, totals = M.extract(vol, cfg, vcap, tcap)
        assert totals == (nv, nt) and v.tobytes() == want_v[:vcap].tobytes() and t.tobytes() == want_t[:tcap].tobytes()
    assert int(want_t["v"].max()) > nv // 2                          # cut triangles still carry the full numbering


def test_scan_defers_overflow_above_two_to_the_32_vertices():
    """The host build of the scan's comparison over synthetic chunk counts: 1792 vertices per chunk (7 per voxel) is the most a
    chunk can hold; 2396746 chunks of them exceed 2^32 - 1, one fewer does not. The sum is carried in 64 bits."""
    L = MC.emu()
    totals = np.zeros(2, np.int64)
    n = -(-(1 << 32) // 1792)
    vc = np.full(n, 1792, np.int32)
    tc = np.full(n, 3072, np.int32)
    big = 1 << 40
    assert L.emu_mesh_scan(vc.ctypes.data, tc.ctypes.data, n, big, big, None, None, totals.ctypes.data) == 2
    assert tuple(totals) == (n * 1792, n * 3072) and totals[0] > 0xFFFFFFFF
    assert L.emu_mesh_scan(vc.ctypes.data, tc.ctypes.data, n - 1, big, big, None, None, totals.ctypes.data) == 0
    assert totals[0] == (n - 1) * 1792 <= 0xFFFFFFFF
    vc[:] = 0
    vc[:3] = (0x7FFFFFFF, 0x7FFFFFFF, 1)                             # 2^32 - 1 exactly, then one more
    assert L.emu_mesh_scan(vc.ctypes.data, tc.ctypes.data, 3, big, big, None, None, totals.ctypes.data) == 0 and totals[0] == 0xFFFFFFFF
    vc[3] = 1
    assert L.emu_mesh_scan(vc.ctypes.data, tc.ctypes.data, 4, big, big, None, None, totals.ctypes.data) == 2
    assert L.emu_mesh_scan(vc.ctypes.data, tc.ctypes.data, 4, 10, big, None, None, totals.ctypes.data) == 3      # and too small
    assert L.emu_mesh_scan(vc.ctypes.data, tc.ctypes.data, 1, 0x7FFFFFFF, 3071, None, None, totals.ctypes.data) == 1


def test_ref_accuracy_of_diagonal_vertices_on_the_analytic_scene():
    """The three-pose scene of tests/tsdf_cases.py; the metric is the distance of each vertex on a DIAGONAL edge (dir 3, 5, 6,
    7) to the nearer of the plane and the sphere. Measured with this restatement at voxel 0.1: 2204 diagonal vertices, median
    0.00067, 95th percentile 0.01878, maximum 0.0716 (axis vertices: 0.00066 and 0.0199, tests/test_tsdf_host.py). Asserted: twice the measured
    values; the margin covers nothing but a different libm."""
    cfg, vol = MC.scene()
    v = MC.ref("scene", vol, cfg)[0]
    diag = v[~np.isin(v["dir"], (1, 2, 4))]
    d = TC.surface_distance(diag["X"])
    med, p95 = np.median(d), np.percentile(d, 95)
    print("diagonal vertices %d, median %.5f, p95 %.5f, max %.5f" % (len(diag), med, p95, d.max()))
    assert len(diag) > 1000 and med <= 2 * 0.00067 and p95 <= 2 * 0.01878



def test_mesh_kernels_cross_compile_without_scratch():
    """From the compiler's resource metadata of the gfx950 listing: no private scratch in any kernel of the file and no float
    atomics anywhere; the only atomic is the deferred-error OR of the scan."""
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "tsdf_mesh.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "tsdf_mesh.hip")])
    text = open(path).read()
    for k in KERNELS:
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        hist, _, _ = S.stats(body)
        atomics = [op for op in hist if op.startswith(("global_atomic", "buffer_atomic", "flat_atomic", "ds_add", "ds_or"))]
        assert not any("f32" in op or "f64" in op for op in atomics), k
        assert atomics == ([] if k != "k_mesh_scan" else [op for op in atomics if op.startswith("global_atomic_or")]), (k, atomics)
    body, _ = S.kernel_body(text, "k_mesh_emit")
    assert S.stats(body)[0]["v_div_fixup_f32"] == 7                  # alpha of each of the seven edges, correctly rounded


def test_mesh_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "tsdf_mesh.hip" in src_line and "tsdf_mesh_table.inc" in mk
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "tsdf_mesh.hip")).read()
    assert "getenv" not in src and "asm" not in src.replace("aria_slam_amd", "")
