"""Shared inputs of the path-planning tests (test_nav_host.py, test_nav_kernel_emulation.py, test_gpu_nav.py): the grids the
device tests run, their goals and queries, and the restatement's results on them (aria_slam_amd/nav_ref.py), computed once
per process and handed out read-only. A grid of nu x nv cells is the x-z plane of a volume of (nu, 8, nv) voxels with
up_axis = 1 unless a case says otherwise."""
import collections
import functools

import numpy as np

from aria_slam_amd import nav_ref as R

GUARD = 0x5A
GUARD32 = 0x5A5A5A5A


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def grid_config(nu, nv, **kw):
    d = dict(dims=(nu, 8, nv), up_axis=1, band=(0, 8), clear_radius=1, block_d2=1, soft_d2=4, penalty=7, unknown_penalty=3)
    d.update(kw)
    return R.config(**d)


Case = collections.namedtuple("Case", "cfg cells goals queries d2 cost fields")


def _case(cfg, cells, goals, queries):
    cells = np.ascontiguousarray(cells, np.uint8)
    goals = np.asarray(goals, np.int32).reshape(-1, 2)
    queries = np.asarray(queries, np.int32).reshape(-1, 3)
    d2, cost = R.build(cells, cfg)
    fields = R.solve(cost, goals)
    return Case(cfg, *_ro(cells, goals, queries, d2, cost, fields))


def _free_cells(cost):
    v, u = np.nonzero(cost != R.BLOCKED)
    return np.stack([u, v], axis=1)


# ---- the 8 x 8 hand-made grid of test_nav_host.py ------------------------------------------------------------------------
HAND_ROWS = ("........",
             "..#.....",
             "..#..?..",
             "..####..",
             "........",
             ".#......",
             "........",
             "......#.")                                           # row v from the top, u from the left; # OCCUPIED, ? UNKNOWN


def rows_to_cells(rows):
    return np.array([[{".": 0, "#": 1, "?": 2}[ch] for ch in row] for row in rows], np.uint8)


@functools.lru_cache(maxsize=None)
def hand():
    cfg = grid_config(8, 8)
    return _case(cfg, rows_to_cells(HAND_ROWS), [(7, 0)], [(0, 7, 0), (3, 2, 0), (2, 1, 0)])


# ---- random obstacles --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_grid(nu, nv, seed=5, n_goals=5, n_queries=40, **kw):
    """About 25 % OCCUPIED cells and a few UNKNOWN ones from a fixed seed; goals on free cells; queries from every kind of cell,
    one of them outside the grid and one with a goal index outside [0, G)."""
    rng = np.random.default_rng(seed)
    cfg = grid_config(nu, nv, **kw)
    cells = (rng.random((nv, nu)) < 0.25).astype(np.uint8)
    cells[(rng.random((nv, nu)) < 0.05) & (cells == 0)] = 2
    cost = R.build(cells, cfg)[1]
    free = _free_cells(cost)
    goals = free[rng.choice(len(free), n_goals, replace=False)]
    q = np.stack([rng.integers(0, nu, n_queries), rng.integers(0, nv, n_queries), rng.integers(0, n_goals, n_queries)], axis=1)
    q[0] = (nu, 0, 0)
    q[1] = (0, 0, n_goals)
    q[2] = (-1, 3, 0)
    q[3] = (goals[1][0], goals[1][1], 1)                             # a start that is its goal
    return _case(cfg, cells, goals, q)


def path_moves(path, nu):
    """The (du, dv) of every step of a path of linear indices."""
    p = np.asarray(path, np.int64)
    return np.stack([p[1:] % nu - p[:-1] % nu, p[1:] // nu - p[:-1] // nu], axis=1)


def refused_diagonals(cost):
    """The number of (cell, diagonal move) pairs whose target is free and inside and which the corner rule alone refuses."""
    nv, nu = cost.shape
    mv = R.allowed_moves(cost)
    n = 0
    for m in range(4, 8):
        du, dv = R.MOVES[m]
        for v in range(max(0, -dv), min(nv, nv - dv)):
            for u in range(max(0, -du), min(nu, nu - du)):
                if cost[v, u] != R.BLOCKED and cost[v + dv, u + du] != R.BLOCKED and not mv[v, u] >> m & 1:
                    n += 1
    return n


# ---- the empty grid: only the move order decides -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def empty():
    cfg = grid_config(16, 16, penalty=0)
    rng = np.random.default_rng(16)
    goals = [(0, 0), (15, 15), (7, 9), (15, 0)]
    q = np.stack([rng.integers(0, 16, 40), rng.integers(0, 16, 40), rng.integers(0, 4, 40)], axis=1)
    return _case(cfg, np.zeros((16, 16), np.uint8), goals, q)


# ---- the serpentine: one corridor through 64 x 64 cells -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def serpentine():
    """Every odd row is a wall with one gap, at the right end and the left end in turn; no clearance (R = 0)."""
    cfg = grid_config(64, 64, clear_radius=0, block_d2=0, soft_d2=1, penalty=0)
    cells = np.zeros((64, 64), np.uint8)
    for v in range(1, 63, 2):
        cells[v, :] = 1
        cells[v, 63 if v % 4 == 1 else 0] = 0
    return _case(cfg, cells, [(63, 62), (0, 0)], [(0, 0, 0), (63, 62, 1), (5, 30, 0), (5, 1, 0)])


# ---- clearance and penalties ---------------------------------------------------------------------------------------------
PROBE = (16, 16)
CLEAR_PARAMS = {0: dict(block_d2=1, soft_d2=1, penalty=30), 1: dict(block_d2=2, soft_d2=4, penalty=30), 8: dict(block_d2=9, soft_d2=49, penalty=30)}


@functools.lru_cache(maxsize=None)
def clearance_case(radius, allow_unknown):
    """32 x 32: obstacles on the border and in the corners, one at distance exactly R from the probe cell along u (inside its
    window) and one at distance R + 1 along v (outside it), a block of UNKNOWN cells."""
    cfg = grid_config(32, 32, clear_radius=radius, allow_unknown=allow_unknown, unknown_penalty=11, **CLEAR_PARAMS[radius])
    cells = np.zeros((32, 32), np.uint8)
    for u, v in ((0, 0), (31, 0), (0, 31), (31, 31), (0, 5), (31, 20), (10, 0), (15, 31), (5, 26)):
        cells[v, u] = 1
    if radius > 0:
        cells[PROBE[1], PROBE[0] + radius] = 1
    cells[PROBE[1] + radius + 1, PROBE[0]] = 1
    cells[2:9, 20:27] = 2
    rng = np.random.default_rng(32 + radius)
    goals = [(3, 3), (28, 28), (23, 5)]
    q = np.stack([rng.integers(0, 32, 24), rng.integers(0, 32, 24), rng.integers(0, 3, 24)], axis=1)
    return _case(cfg, cells, goals, q)


# ---- field storage: a plane that cannot sit in LDS ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big():
    """256 x 256 with rectangular obstacles and a long wall; G = 4."""
    cfg = grid_config(256, 256, clear_radius=3, block_d2=4, soft_d2=16, penalty=9)
    rng = np.random.default_rng(256)
    cells = np.zeros((256, 256), np.uint8)
    for _ in range(40):
        u, v, w, h = rng.integers(0, 240), rng.integers(0, 240), rng.integers(2, 16), rng.integers(2, 16)
        cells[v:v + h, u:u + w] = 1
    cells[128, 10:256] = 1
    cells[60:70, 200:230] = 2
    cells[0:8, 0:8] = 0
    cells[248:256, 248:256] = 0
    goals = [(2, 2), (252, 252), (2, 252), (252, 2)]
    q = np.stack([rng.integers(0, 256, 16), rng.integers(0, 256, 16), rng.integers(0, 4, 16)], axis=1)
    q[0] = (252, 252, 0)
    return _case(cfg, cells, goals, q)


# ---- the default plane: the LDS form above 64 KiB ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def default_plane():
    """256 x 128, the plane of the default volume under the default radii and penalties: 131 584 B of LDS per goal. Rooms with
    doors wide enough for block_d2 = 16, a closed room, a block of UNKNOWN cells; G = 3."""
    cfg = R.config(dims=(256, 8, 128), up_axis=1, band=(0, 8))
    assert 64 * 1024 < 4 * 257 * 128 <= 160 * 1024 - 64
    rng = np.random.default_rng(128)
    cells = np.zeros((128, 256), np.uint8)
    for u in range(32, 256, 32):
        cells[:, u] = 1
        for v0 in range(0, 128, 32):
            d = v0 + int(rng.integers(4, 16))
            cells[d:d + 12, u] = 0
    for v in range(32, 128, 32):
        cells[v, :] = 1
        for u0 in range(0, 256, 32):
            d = u0 + int(rng.integers(4, 16))
            cells[v, d:d + 12] = 0
    cells[64:97, 96] = cells[64:97, 128] = cells[64, 96:129] = cells[96, 96:129] = 1        # a room without a door
    cells[10:20, 200:215] = 2
    goals = [(8, 8), (250, 120), (112, 80)]                          # the third sits in the closed room
    q = np.stack([rng.integers(0, 256, 24), rng.integers(0, 128, 24), rng.integers(0, 3, 24)], axis=1)
    q[0] = (250, 120, 0)
    q[1] = (110, 82, 2)
    return _case(cfg, cells, goals, q)


# ---- many goals -----------------------------------------------------------------------------------------------------------
N_MANY = 320


@functools.lru_cache(maxsize=None)
def many():
    """16 x 16 and 320 goals, more than the card has CUs: a duplicate goal, a goal on a blocked cell, a goal outside the grid
    and a goal that is its own start among them."""
    rng = np.random.default_rng(320)
    cfg = grid_config(16, 16, max_goals=N_MANY)
    cells = (rng.random((16, 16)) < 0.2).astype(np.uint8)
    cost = R.build(cells, cfg)[1]
    free = _free_cells(cost)
    goals = free[rng.integers(0, len(free), N_MANY)].copy()
    blocked_v, blocked_u = np.nonzero(cost == R.BLOCKED)
    goals[7] = goals[3]                                              # a duplicate
    goals[11] = (blocked_u[0], blocked_v[0])                         # on a blocked cell
    goals[13] = (16, 2)                                              # outside the grid
    q = np.stack([rng.integers(0, 16, 64), rng.integers(0, 16, 64), rng.integers(0, N_MANY, 64)], axis=1)
    q[0] = (goals[3][0], goals[3][1], 7)                             # the duplicate's field, from the goal itself
    q[1] = (free[0][0], free[0][1], 11)
    q[2] = (free[0][0], free[0][1], 13)
    q[3] = (goals[319][0], goals[319][1], 319)                       # a goal that is its own start
    return _case(cfg, cells, goals, q)


# ---- rule 2 on a hand-built 8 x 8 x 8 volume -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_volume():
    """(cfg, volume [8, 8, 8], wanted cells [8, 8]) with up_axis = 1, band [2, 5), min_weight 3, occ_tsdf 0.25, occ_count 2,
    free_count 2. Column (u, v) = (i, k) holds what its comment says."""
    from aria_slam_amd.tsdf_ref import VOXEL_DTYPE
    cfg = R.config(dims=(8, 8, 8), up_axis=1, band=(2, 5), min_weight=3, occ_tsdf=0.25, occ_count=2, free_count=2, clear_radius=1,
                   block_d2=1, soft_d2=4)
    vol = np.zeros((8, 8, 8), VOXEL_DTYPE)
    want = np.full((8, 8), R.UNKNOWN, np.uint8)

    def put(i, k, j, tsdf, weight):
        vol[k, j, i] = (tsdf, weight, 0, 0)

    # (0, 0): two solid voxels inside the band -> OCCUPIED
    put(0, 0, 2, -0.5, 3); put(0, 0, 4, 0.0, 9); want[0, 0] = R.OCCUPIED
    # (1, 0): solid voxels at j = 1 and j = 5, just outside the band, and one inside: one solid, one seen -> UNKNOWN
    put(1, 0, 1, -1.0, 9); put(1, 0, 5, -1.0, 9); put(1, 0, 3, -1.0, 9); want[0, 1] = R.UNKNOWN
    # (2, 0): j = 2 and j = 4, the band's included edges, both seen and not solid -> FREE
    put(2, 0, 2, 0.5, 3); put(2, 0, 4, 1.0, 3); want[0, 2] = R.FREE
    # (3, 0): two solid voxels but one with weight one below min_weight: one solid, one seen -> UNKNOWN
    put(3, 0, 2, -0.5, 2); put(3, 0, 3, -0.5, 3); want[0, 3] = R.UNKNOWN
    # (4, 0): tsdf == occ_tsdf is not solid: two seen, one solid -> FREE
    put(4, 0, 2, 0.25, 3); put(4, 0, 3, 0.2, 3); want[0, 4] = R.FREE
    # (5, 1): three solid -> OCCUPIED, although free_count is met as well
    put(5, 1, 2, -0.1, 5); put(5, 1, 3, -0.1, 5); put(5, 1, 4, -0.1, 5); want[1, 5] = R.OCCUPIED
    # (6, 7): solid only outside the band, two seen inside -> FREE
    put(6, 7, 0, -1.0, 9); put(6, 7, 7, -1.0, 9); put(6, 7, 2, 0.9, 4); put(6, 7, 3, 0.9, 4); want[7, 6] = R.FREE
    # (7, 7): NaN is not below occ_tsdf: two seen, none solid -> FREE
    put(7, 7, 2, np.nan, 4); put(7, 7, 3, np.nan, 4); want[7, 7] = R.FREE
    return cfg, _ro(vol), _ro(want)


# ---- the chain: the TSDF scene, one plan per up_axis ----------------------------------------------------------------------
CHAIN_BANDS = {0: (15, 19), 1: (10, 14), 2: (5, 9)}                  # each cuts the sphere of tsdf_cases


@functools.lru_cache(maxsize=None)
def chain(up_axis):
    """(case, volume): the cells of tsdf_cases.ref_scene()'s volume under a band that cuts the sphere, goals and queries on
    its free cells."""
    import tsdf_cases as TC
    tcfg, vol, _ = TC.ref_scene()
    cfg = R.config(dims=tcfg.dims, up_axis=up_axis, band=CHAIN_BANDS[up_axis], min_weight=tcfg.min_weight, voxel=tcfg.voxel,
                   origin=tcfg.origin, clear_radius=2, block_d2=2, soft_d2=9, penalty=12, unknown_penalty=5)
    cells = R.cells_from_volume(vol, cfg)
    nu, nv = R.grid_shape(cfg)
    cost = R.build(cells, cfg)[1]
    free = _free_cells(cost)
    rng = np.random.default_rng(40 + up_axis)
    goals = np.concatenate([free[[0, -1]], free[rng.choice(len(free), 2, replace=False)]])
    q = np.stack([rng.integers(0, nu, 20), rng.integers(0, nv, 20), rng.integers(0, 4, 20)], axis=1)
    q[0] = (free[-1][0], free[-1][1], 0)                             # across the scene
    q[1] = (free[0][0], free[0][1], 1)
    return _case(cfg, cells, goals, q), vol


_cache = {}


def traced(name, case, path_cap, fill=0):
    """(records, paths, truncated) of the restatement for a case, computed once per (name, path_cap, fill)."""
    key = (name, path_cap, fill)
    if key not in _cache:
        paths = np.full((len(case.queries), path_cap), fill, np.int32)
        rec, paths, trunc = R.trace(case.cost, case.d2, case.fields, case.goals, case.queries, path_cap, paths)
        _cache[key] = (*_ro(rec, paths), trunc)
    return _cache[key]
