"""NumPy restatement of the path-planning stage (include/aria_orb_hip.h, "path planning"): a 2-D traversability grid
collapsed out of a height band of the TSDF volume, an exact clearance field and an integer cost map, exact cost-to-go
fields for a batch of goals, and paths traced for a batch of queries. The reference has no code for it (its roadmap items
H20 and H22 sit on such a map), so this file IS the definition and the device equals it bit for bit.

All arithmetic is in integers except the one fp32 comparison of rule 2, so there is no tolerance anywhere. Arrays over the
grid are indexed [v, u]: cell (u, v) has the linear index c = v*nu + u."""
import heapq
from collections import namedtuple

import numpy as np

from .tsdf_ref import VOXEL_DTYPE

RECORD_DTYPE = np.dtype([("cost", "<i4"), ("n_cells", "<i4"), ("min_d2", "<i4"), ("status", "<i4")])   # aria_nav_record, 16 bytes

FREE, OCCUPIED, UNKNOWN = 0, 1, 2
OK, UNREACHABLE, OUT_OF_GRID, TRUNCATED = 0, 1, 2, 3
INF = 0x7FFFFFFF
BLOCKED = 0xFFFF
MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))       # rule 5, in this order
BASE = (10, 10, 10, 10, 14, 14, 14, 14)

DEFAULTS = dict(dims=(256, 256, 128), up_axis=1, band=None, min_weight=2, occ_tsdf=0.0, occ_count=1, free_count=1,
                clear_radius=8, block_d2=16, soft_d2=64, penalty=20, unknown_penalty=10, allow_unknown=1, max_goals=256,
                voxel=0.05, origin=(-6.4, -6.4, 0.0))

Config = namedtuple("Config", "dims up_axis band min_weight occ_tsdf occ_count free_count clear_radius block_d2 soft_d2 "
                              "penalty unknown_penalty allow_unknown max_goals voxel origin")

f32 = np.float32


def default_band(n_up):
    """[n/2 - 8, n/2 + 16) cut to the axis: the default of a geometry (the C default is this at ny = 256)."""
    return (max(n_up // 2 - 8, 0), min(n_up // 2 + 16, n_up))


def config(**kw):
    """A Config from DEFAULTS and the overrides; raises ValueError where aria_nav_create returns ARIA_E_INVALID."""
    d = dict(DEFAULTS)
    d.update(kw)
    dims = tuple(int(v) for v in d["dims"])
    up = int(d["up_axis"])
    ok = len(dims) == 3 and all(8 <= n <= 1024 and n % 8 == 0 for n in dims) and up in (0, 1, 2)
    if not ok:
        raise ValueError("invalid path-planning configuration")
    band = default_band(dims[up]) if d["band"] is None else tuple(int(v) for v in d["band"])
    c = Config(dims=dims, up_axis=up, band=band, min_weight=int(d["min_weight"]), occ_tsdf=f32(d["occ_tsdf"]),
               occ_count=int(d["occ_count"]), free_count=int(d["free_count"]), clear_radius=int(d["clear_radius"]),
               block_d2=int(d["block_d2"]), soft_d2=int(d["soft_d2"]), penalty=int(d["penalty"]),
               unknown_penalty=int(d["unknown_penalty"]), allow_unknown=int(d["allow_unknown"]), max_goals=int(d["max_goals"]),
               voxel=f32(d["voxel"]), origin=tuple(f32(v) for v in d["origin"]))
    cap = (c.clear_radius + 1) ** 2 if 0 <= c.clear_radius <= 64 else -1
    ok = len(band) == 2 and 0 <= band[0] < band[1] <= dims[up]
    ok = ok and 1 <= c.min_weight <= 65535 and np.isfinite(c.occ_tsdf) and 1 <= c.occ_count <= 1024 and 1 <= c.free_count <= 1024
    ok = ok and 0 <= c.clear_radius <= 64 and 0 <= c.block_d2 <= c.soft_d2 <= cap and c.soft_d2 >= 1
    ok = ok and 0 <= c.penalty <= 1000 and 0 <= c.unknown_penalty <= 1000 and c.allow_unknown in (0, 1)
    ok = ok and 1 <= c.max_goals <= 65535 and np.isfinite(c.voxel) and c.voxel > 0 and all(np.isfinite(v) for v in c.origin)
    if not ok:
        raise ValueError("invalid path-planning configuration")
    return c


def plane_axes(up_axis):
    """(U, V): the two volume axes other than up_axis, ascending."""
    return tuple(a for a in range(3) if a != up_axis)


def grid_shape(cfg):
    """(nu, nv)."""
    U, V = plane_axes(cfg.up_axis)
    return cfg.dims[U], cfg.dims[V]


def cells_from_volume(vol, cfg):
    """Rule 2. vol: VOXEL_DTYPE [nz, ny, nx]. Returns uint8 [nv, nu]."""
    vol = np.asarray(vol)
    assert vol.dtype == VOXEL_DTYPE and vol.shape == cfg.dims[::-1]
    ax = 2 - cfg.up_axis                                             # the array axis of the volume axis
    sl = [slice(None)] * 3
    sl[ax] = slice(cfg.band[0], cfg.band[1])
    band = vol[tuple(sl)]
    seen = band["weight"] >= cfg.min_weight
    solid = seen & (band["tsdf"] < cfg.occ_tsdf)                     # an fp32 compare
    n_seen, n_solid = seen.sum(axis=ax), solid.sum(axis=ax)          # what is left is [V, U]: the larger volume axis comes first
    return np.where(n_solid >= cfg.occ_count, OCCUPIED, np.where(n_seen >= cfg.free_count, FREE, UNKNOWN)).astype(np.uint8)


def check_cells(cells, cfg):
    """The cells as uint8 [nv, nu]; ValueError for a wrong shape or a value above 2 (the host form's ARIA_E_INVALID)."""
    nu, nv = grid_shape(cfg)
    cells = np.asarray(cells)
    if cells.shape != (nv, nu) or cells.dtype != np.uint8 or (cells > 2).any():
        raise ValueError("cells are uint8 [nv, nu] with values 0, 1, 2")
    return cells


def clearance(cells, cfg):
    """Rule 3, the brute-force window: uint16 [nv, nu]."""
    R = cfg.clear_radius
    nv, nu = cells.shape
    occ = cells == OCCUPIED
    d2 = np.full((nv, nu), (R + 1) * (R + 1), np.int64)
    for dv in range(-R, R + 1):
        for du in range(-R, R + 1):
            # the cells c whose neighbour (u + du, v + dv) is inside the grid
            v0, v1, u0, u1 = max(0, -dv), min(nv, nv - dv), max(0, -du), min(nu, nu - du)
            if v0 >= v1 or u0 >= u1:
                continue
            hit = occ[v0 + dv:v1 + dv, u0 + du:u1 + du]
            view = d2[v0:v1, u0:u1]
            np.minimum(view, np.where(hit, du * du + dv * dv, view), out=view)
    return d2.astype(np.uint16)


def costs(cells, d2, cfg):
    """Rule 4: uint16 [nv, nu], 0xFFFF = blocked."""
    d2 = d2.astype(np.int64)
    blocked = (cells == OCCUPIED) | (d2 < cfg.block_d2) | ((cells == UNKNOWN) & (cfg.allow_unknown == 0))
    pen = np.where(d2 < cfg.soft_d2, cfg.penalty * (cfg.soft_d2 - d2) // cfg.soft_d2, 0) + np.where(cells == UNKNOWN, cfg.unknown_penalty, 0)
    return np.where(blocked, BLOCKED, pen).astype(np.uint16)


def build(cells, cfg):
    """(clearance, costs) of a cell grid."""
    d2 = clearance(cells, cfg)
    return d2, costs(cells, d2, cfg)


def allowed_moves(cost):
    """Rule 5: uint8 [nv, nu], bit m set when move m out of the cell is allowed (the cell itself may be blocked)."""
    nv, nu = cost.shape
    free = np.zeros((nv + 2, nu + 2), bool)                          # a border of "not allowed" around the grid
    free[1:-1, 1:-1] = cost != BLOCKED
    at = lambda du, dv: free[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]   # noqa: E731
    out = np.zeros((nv, nu), np.uint8)
    for m, (du, dv) in enumerate(MOVES):
        ok = at(du, dv)
        if du and dv:
            ok = ok & at(du, 0) & at(0, dv)
        out |= (ok.astype(np.uint8) << m).astype(np.uint8)
    return out


def _goal_ok(cost, goal):
    nv, nu = cost.shape
    gu, gv = int(goal[0]), int(goal[1])
    return 0 <= gu < nu and 0 <= gv < nv and cost[gv, gu] != BLOCKED


def field(cost, goal):
    """Rule 6 by a heap Dijkstra from the goal: int32 [nv, nu]. A move c -> b and the move b -> c are allowed together when
    neither cell is blocked (the two corner cells of a diagonal are the same), so the search walks the moves backwards."""
    nv, nu = cost.shape
    D = np.full(nv * nu, INF, np.int64)
    if not _goal_ok(cost, goal):
        return D.reshape(nv, nu).astype(np.int32)
    mv = allowed_moves(cost).reshape(-1).tolist()
    cl = cost.reshape(-1).tolist()
    dist = [INF] * (nv * nu)
    g = int(goal[1]) * nu + int(goal[0])
    dist[g] = 0
    heap = [(0, g)]
    offs = [dv * nu + du for du, dv in MOVES]
    while heap:
        d, b = heapq.heappop(heap)
        if d != dist[b]:
            continue
        mb, pb = mv[b], cl[b]
        for m in range(8):
            if mb >> m & 1:                                          # b -> c allowed, so is c -> b
                c = b + offs[m]
                if cl[c] != BLOCKED:
                    cand = d + BASE[m] + pb                          # step(c -> b) = base + pen(b)
                    if cand < dist[c]:
                        dist[c] = cand
                        heapq.heappush(heap, (cand, c))
    return np.array(dist, np.int64).reshape(nv, nu).astype(np.int32)


def field_sweeps(cost, goal):
    """Rule 6 literally: D(g) = 0, every other cell INF, and all cells replaced at once by the minimum over their allowed moves
    until nothing changes. Returns (field, sweeps)."""
    nv, nu = cost.shape
    D = np.full((nv, nu), INF, np.int64)
    if not _goal_ok(cost, goal):
        return D.astype(np.int32), 0
    mv = allowed_moves(cost)
    pen = np.where(cost == BLOCKED, 0, cost).astype(np.int64)
    free = cost != BLOCKED
    gu, gv = int(goal[0]), int(goal[1])
    D[gv, gu] = 0
    sweeps = 0
    while True:
        pad = np.full((nv + 2, nu + 2), INF, np.int64)
        pad[1:-1, 1:-1] = D + np.where(D < INF, pen, 0)              # step + D(b) = base + (pen(b) + D(b))
        new = D.copy()
        for m, (du, dv) in enumerate(MOVES):
            nb = pad[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]
            ok = ((mv >> m) & 1).astype(bool) & free & (nb < INF)
            new = np.where(ok, np.minimum(new, nb + BASE[m]), new)
        new[gv, gu] = 0
        sweeps += 1
        if (new == D).all():
            return D.astype(np.int32), sweeps
        if sweeps > nu * nv:
            raise RuntimeError("the sweeps did not settle")
        D = new


def solve(cost, goals):
    """int32 [G, nv, nu]: one field per goal (u, v)."""
    goals = np.asarray(goals, np.int32).reshape(-1, 2)
    nv, nu = cost.shape
    out = np.zeros((len(goals), nv, nu), np.int32)
    for k, g in enumerate(goals):
        out[k] = field(cost, g)
    return out


def trace(cost, d2, fields, goals, queries, path_cap, paths=None):
    """Rule 7. queries: int32 [Q, 3] (su, sv, goal_index). Returns (records [Q], paths [Q, path_cap], truncated): `paths`
    is written into when given (what is not written keeps its bytes), else starts at zero; truncated = some query has status 3
    (ARIA_E_OUTPUT_TOO_SMALL is then deferred)."""
    nv, nu = cost.shape
    goals = np.asarray(goals, np.int32).reshape(-1, 2)
    queries = np.asarray(queries, np.int32).reshape(-1, 3)
    G, Q = len(goals), len(queries)
    rec = np.zeros(Q, RECORD_DTYPE)
    if paths is None:
        paths = np.zeros((Q, path_cap), np.int32)
    mv = allowed_moves(cost)
    for q, (su, sv, gi) in enumerate(queries.tolist()):
        inside = 0 <= su < nu and 0 <= sv < nv and 0 <= gi < G
        if inside:
            gu, gv = (int(x) for x in goals[gi])
            inside = 0 <= gu < nu and 0 <= gv < nv
        if not inside:
            rec[q] = (INF, 0, 0, OUT_OF_GRID)
            continue
        D = fields[gi]
        if D[sv, su] == INF:
            rec[q] = (INF, 0, 0, UNREACHABLE)
            continue
        u, v, n, lo = su, sv, 0, int(d2[sv, su])
        while True:
            if n < path_cap:
                paths[q, n] = v * nu + u
            n += 1
            lo = min(lo, int(d2[v, u]))
            if (u, v) == (gu, gv):
                break
            for m, (du, dv) in enumerate(MOVES):
                if mv[v, u] >> m & 1 and BASE[m] + int(cost[v + dv, u + du]) + int(D[v + dv, u + du]) == int(D[v, u]):
                    u, v = u + du, v + dv
                    break
            else:
                raise RuntimeError("no move continues the path: the field is not rule 6's")
        rec[q] = (int(D[sv, su]), n, lo, TRUNCATED if n > path_cap else OK)
    return rec, paths, bool((rec["status"] == TRUNCATED).any())


def cell_of(X, cfg):
    """World points [n, 3] to cells [n, 2] (u, v): floor((x - origin) / voxel) in fp32 on the two plane axes."""
    X = np.asarray(X, f32).reshape(-1, 3)
    U, V = plane_axes(cfg.up_axis)
    out = np.zeros((len(X), 2), np.int32)
    for k, a in enumerate((U, V)):
        out[:, k] = np.floor((X[:, a] - f32(cfg.origin[a])) / cfg.voxel).astype(np.int32)
    return out


def centre_of(cells, cfg):
    """Cells [n, 2] (u, v) to world points fp32 [n, 3]: the TSDF stage's voxel centre origin + ((float)i + 0.5f) * voxel on the
    plane axes, and the middle of the band on up_axis: origin + ((float)(band0 + band1) * 0.5f) * voxel."""
    cells = np.asarray(cells, np.int32).reshape(-1, 2)
    U, V = plane_axes(cfg.up_axis)
    out = np.zeros((len(cells), 3), f32)
    for k, a in enumerate((U, V)):
        out[:, a] = f32(cfg.origin[a]) + (cells[:, k].astype(f32) + f32(0.5)) * cfg.voxel
    out[:, cfg.up_axis] = f32(cfg.origin[cfg.up_axis]) + (f32(cfg.band[0] + cfg.band[1]) * f32(0.5)) * cfg.voxel
    return out


def field_bytes(nu, nv, max_goals):
    return 4 * nu * nv * max_goals
