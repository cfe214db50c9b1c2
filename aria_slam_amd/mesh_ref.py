"""NumPy restatement of the mesh stage (include/aria_orb_hip.h, "mesh of the volume"): the aria_tsdf_voxel records of the
dense depth fusion contoured into a triangle mesh by marching tetrahedra on the Kuhn split of every cell. The reference has
no code for it, so this file IS the definition and the device equals it byte for byte.

Every float operation is fp32 with one rounding per operation, in the order the header writes it. The 6 x 16 table is
derived here, when the module is imported, from the orientation rule alone; aria_slam_amd/csrc/tsdf_mesh_table.inc holds the
same words as constants (table_text() writes that file's body)."""
from collections import namedtuple

import numpy as np

VOXEL_DTYPE = np.dtype([("tsdf", "<f4"), ("weight", "<u2"), ("gray", "u1"), ("reserved", "u1")])       # aria_tsdf_voxel, 8 bytes
VERTEX_DTYPE = np.dtype([("X", "<f4", (3,)), ("gray", "u1"), ("dir", "u1"), ("weight", "<u2")])        # aria_mesh_vertex, 16 bytes
TRIANGLE_DTYPE = np.dtype([("v", "<u4", (3,))])                                                        # aria_mesh_triangle, 12 bytes

DEFAULTS = dict(dims=(256, 256, 128), voxel=0.05, origin=(-6.4, -6.4, 0.0), min_weight=2)
Config = namedtuple("Config", "dims voxel origin min_weight")

f32 = np.float32

# tetrahedron p: the axis permutations in the order xyz, xzy, yxz, yzx, zxy, zyx; corners (0, 2^p0, 2^p0 + 2^p1, 7)
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TET_CORNERS = tuple((0, 1 << p[0], (1 << p[0]) + (1 << p[1]), 7) for p in PERMS)


def config(**kw):
    """A Config from DEFAULTS and the overrides; raises ValueError where aria_mesh_create returns ARIA_E_INVALID."""
    d = dict(DEFAULTS)
    d.update(kw)
    c = Config(dims=tuple(int(v) for v in d["dims"]), voxel=f32(d["voxel"]), origin=tuple(f32(v) for v in d["origin"]),
               min_weight=int(d["min_weight"]))
    ok = len(c.dims) == 3 and all(8 <= n <= 1024 and n % 8 == 0 for n in c.dims)
    ok = ok and np.isfinite(c.voxel) and c.voxel > 0 and len(c.origin) == 3 and all(np.isfinite(v) for v in c.origin)
    ok = ok and 1 <= c.min_weight <= 65535
    if not ok:
        raise ValueError("invalid mesh configuration")
    return c


def _corner_xyz(q):
    return np.array([q & 1, (q >> 1) & 1, (q >> 2) & 1], np.float64)


def _derive_table():
    """TABLE[p][mask]: the triangles of tetrahedron p under the 4-bit inside mask (bit t = tetrahedron corner t inside), each
    a triple of edges (lower cell corner, d): rule 4 of the header."""
    table = []
    for corners in TET_CORNERS:
        row = []
        for mask in range(16):
            ins = [t for t in range(4) if mask >> t & 1]
            out = [t for t in range(4) if not mask >> t & 1]
            if len(ins) in (0, 4):
                row.append(())
                continue
            if len(ins) == 1:
                poly = [(ins[0], o) for o in out]
            elif len(ins) == 3:
                poly = [(i, out[0]) for i in ins]
            else:
                (a, b), (c, d) = ins, out
                poly = [(a, c), (a, d), (b, d), (b, c)]
            mid = [(_corner_xyz(corners[s]) + _corner_xyz(corners[t])) / 2 for s, t in poly]
            want = np.mean([_corner_xyz(corners[t]) for t in out], axis=0) - np.mean([_corner_xyz(corners[t]) for t in ins], axis=0)
            tris = [(0, 1, 2)] if len(poly) == 3 else [(0, 1, 2), (0, 2, 3)]
            if np.dot(np.cross(mid[tris[0][1]] - mid[tris[0][0]], mid[tris[0][2]] - mid[tris[0][0]]), want) <= 0:
                tris = [(t[0], t[2], t[1]) for t in tris]
            for t in tris:
                assert np.dot(np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]]), want) > 0
            edges = []
            for s, t in poly:
                lo, hi = corners[min(s, t)], corners[max(s, t)]
                assert lo & hi == lo and lo != hi and lo <= 6                   # an edge of rule 2 owned by a corner 0..6
                edges.append((lo, hi - lo))
            row.append(tuple(tuple(edges[e] for e in t) for t in tris))
        table.append(tuple(row))
    return tuple(table)


TABLE = _derive_table()
TRIANGLE_COUNTS = tuple(len(t) for t in TABLE[0])


def table_words():
    """The table as the HIP side holds it: 6 x 16 words; bits 0-1 the triangle count, then the edges of the triangles in
    order, six bits each from bit 4: (lower corner << 3) | d."""
    words = []
    for row in TABLE:
        for tris in row:
            w, n = len(tris), 0
            for tri in tris:
                for lo, d in tri:
                    w |= ((lo << 3) | d) << (4 + 6 * n)
                    n += 1
            words.append(w)
    return words


def table_text():
    """The body of aria_slam_amd/csrc/tsdf_mesh_table.inc."""
    w = table_words()
    return "".join("    {" + ", ".join("0x%010xull" % v for v in w[16 * p:16 * p + 16]) + "},\n" for p in range(6))


def centres(cfg):
    """c = origin + ((float)i + 0.5f) * voxel per axis: three fp32 vectors (x over i, y over j, z over k)."""
    return tuple(f32(cfg.origin[a]) + (np.arange(cfg.dims[a], dtype=f32) + f32(0.5)) * cfg.voxel for a in range(3))


def _slices(d, n):
    dx, dy, dz = d & 1, (d >> 1) & 1, (d >> 2) & 1
    nx, ny, nz = n
    return ((slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx)), (slice(dz, nz), slice(dy, ny), slice(dx, nx)))


def _vertices(vol, cfg):
    """(vertices in canonical order, vid[d - 1, k, j, i] = the vertex number of edge (voxel, d) or -1)."""
    nx, ny, nz = cfg.dims
    gx, gy, gz = centres(cfg)
    t, w, g = vol["tsdf"], vol["weight"], vol["gray"]
    seen, inside = w >= cfg.min_weight, t < 0
    lins, recs = [], []
    with np.errstate(all="ignore"):
        for d in range(1, 8):
            sa, sb = _slices(d, cfg.dims)
            hit = seen[sa] & seen[sb] & (inside[sa] != inside[sb])
            k, j, i = np.nonzero(hit)
            ta, tb = t[sa][hit], t[sb][hit]
            alpha = ta / (ta - tb)
            step = alpha * cfg.voxel
            X = np.stack([gx[i], gy[j], gz[k]], axis=1)
            for a in range(3):
                if d >> a & 1:
                    X[:, a] = X[:, a] + step
            v = np.zeros(len(k), VERTEX_DTYPE)
            v["X"] = X
            v["gray"] = np.where(alpha < f32(0.5), g[sa][hit], g[sb][hit])
            v["dir"] = d
            v["weight"] = np.minimum(w[sa][hit], w[sb][hit])
            lins.append((k.astype(np.int64) * ny + j) * nx + i)
            recs.append(v)
    lin, verts = np.concatenate(lins), np.concatenate(recs)
    order = np.lexsort((verts["dir"], lin))
    lin, verts = lin[order], verts[order]
    vid = np.full((7, nz * ny * nx), -1, np.int64)
    vid[verts["dir"].astype(np.int64) - 1, lin] = np.arange(len(verts), dtype=np.int64)
    return verts, vid, lin


def _corner(a, q):
    """a[k, j, i] at corner q of every cell: an array [nz - 1, ny - 1, nx - 1]."""
    bx, by, bz = q & 1, (q >> 1) & 1, (q >> 2) & 1
    nz, ny, nx = a.shape
    return a[bz:bz + nz - 1, by:by + ny - 1, bx:bx + nx - 1]


def live_cells(vol, cfg):
    """bool [nz - 1, ny - 1, nx - 1]: rule 3's live cells."""
    seen = np.asarray(vol)["weight"] >= cfg.min_weight
    live = _corner(seen, 0).copy()
    for q in range(1, 8):
        live &= _corner(seen, q)
    return live


def _triangles(vol, cfg, vid):
    nx, ny, nz = cfg.dims
    inside = vol["tsdf"] < 0
    live = live_cells(vol, cfg)
    ins = [_corner(inside, q) for q in range(8)]
    k, j, i = np.nonzero(live)
    lin = (k.astype(np.int64) * ny + j) * nx + i
    ins = [a[live] for a in ins]
    off = [(q & 1) + ((q >> 1) & 1) * nx + ((q >> 2) & 1) * nx * ny for q in range(8)]
    keys, tris = [], []
    for p, corners in enumerate(TET_CORNERS):
        mask = sum(ins[c].astype(np.int64) << t for t, c in enumerate(corners))
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            if not len(sel):
                continue
            for n, tri in enumerate(TABLE[p][m]):
                v = np.stack([vid[d - 1, lin[sel] + off[lo]] for lo, d in tri], axis=1)
                assert (v >= 0).all()
                keys.append((lin[sel] * 6 + p) * 2 + n)
                tris.append(v)
    if not keys:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.argsort(keys, kind="stable")
    return tris[order], keys[order] // 12


def extract(vol, cfg, vcap=None, tcap=None):
    """(vertices, triangles, (vertex total, triangle total)) of the records vol[k, j, i]: rules 2-6. The arrays are cut to
    the first min(total, cap); the triangles carry the full numbering either way."""
    vol = np.asarray(vol)
    nx, ny, nz = cfg.dims
    assert vol.dtype == VOXEL_DTYPE and vol.shape == (nz, ny, nx)
    verts, vid, _ = _vertices(vol, cfg)
    tri, _ = _triangles(vol, cfg, vid)
    assert len(verts) <= 0xFFFFFFFF
    out = np.zeros(len(tri), TRIANGLE_DTYPE)
    out["v"] = tri
    nv, nt = len(verts), len(out)
    return (verts[:nv if vcap is None else min(nv, vcap)].copy(), out[:nt if tcap is None else min(nt, tcap)].copy(), (nv, nt))


def owners(vol, cfg):
    """(linear index of the voxel that owns each vertex, linear index of corner 0 of the cell each triangle comes from), in
    the order of extract(): what the closure tests need to place an edge in the grid."""
    verts, vid, lin = _vertices(np.asarray(vol), cfg)
    return lin, _triangles(np.asarray(vol), cfg, vid)[1]


def directed_edges(triangles):
    """The 3 n directed edges of triangles [n, 3] as an int64 array [3 n, 2]."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_report(triangles):
    """(number of directed edges that occur more than once, the directed edges whose reverse does not occur [m, 2])."""
    e = directed_edges(triangles)
    if not len(e):
        return 0, e
    key = e[:, 0] << 32 | e[:, 1]
    rev = e[:, 1] << 32 | e[:, 0]
    _, counts = np.unique(key, return_counts=True)
    return int((counts > 1).sum()), e[~np.isin(rev, key)]


def scratch_bytes(nx, ny, nz):
    """What a handle of this geometry keeps on the device: a word per voxel and 24 bytes per chunk of 256 voxels."""
    n = nx * ny * nz
    return 4 * n + 24 * (n // 256)


def algorithmic_bytes(nx, ny, nz, n_vertices, n_triangles):
    """One update + extract: every record read once (8 B), its word written once and read once (8 B), 16 B per vertex and
    12 B per triangle written."""
    return 16 * nx * ny * nz + 16 * n_vertices + 12 * n_triangles
