"""Path planning (include/aria_orb_hip.h, "path planning"): the parts that need no GPU -- exports, layouts, defaults and
validation, and the NumPy restatement (aria_slam_amd/nav_ref.py, which is the definition) on known answers: a hand-made 8 x 8
grid written out literally, the heap Dijkstra against the literal fixed-point sweeps of rule 6, and rule 2 on a hand-built
8 x 8 x 8 volume."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nav_cases as NC   # noqa: E402
from aria_slam_amd import nav_ref as R   # noqa: E402

NAV_SYMBOLS = ["aria_nav_default_config", "aria_nav_create", "aria_nav_destroy", "aria_nav_stream", "aria_nav_check",
               "aria_nav_update_from_volume_device", "aria_nav_set_cells_device", "aria_nav_set_cells", "aria_nav_read_cells",
               "aria_nav_read_clearance", "aria_nav_read_costs", "aria_nav_solve_device", "aria_nav_trace_device", "aria_nav_plan",
               "aria_nav_device_fields", "aria_nav_read_field", "aria_nav_read_rounds", "aria_nav_field_bytes"]
I = R.INF
B = R.BLOCKED
f32 = np.float32


def test_nav_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in NAV_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipPathPlanner" in aria.__all__
    assert "and any alert logic" in header and "any path-planning or alert logic" not in header


def test_nav_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    assert C.sizeof(_lib.NavConfig) == 104
    assert _lib.NAV_RECORD_DTYPE.itemsize == 16 and _lib.NAV_RECORD_DTYPE == R.RECORD_DTYPE
    cfg = _lib.NavConfig()
    L.aria_nav_default_config(C.byref(cfg))
    assert cfg.struct_size == 104 and not cfg.stream
    assert (cfg.nx, cfg.ny, cfg.nz, cfg.up_axis, cfg.band0, cfg.band1) == (256, 256, 128, 1, 120, 144)
    assert (cfg.min_weight, cfg.occ_tsdf, cfg.occ_count, cfg.free_count) == (2, 0.0, 1, 1)
    assert (cfg.clear_radius, cfg.block_d2, cfg.soft_d2, cfg.penalty, cfg.unknown_penalty, cfg.allow_unknown) == (8, 16, 64, 20, 10, 1)
    assert cfg.max_goals == 256 and cfg.voxel == f32(0.05) and tuple(cfg.origin) == (f32(-6.4), f32(-6.4), 0.0)
    d = R.config()
    assert (d.dims, d.up_axis, d.band) == ((256, 256, 128), 1, (120, 144)) and R.grid_shape(d) == (256, 128)
    assert (d.min_weight, d.occ_tsdf, d.occ_count, d.free_count, d.clear_radius, d.block_d2, d.soft_d2, d.penalty, d.unknown_penalty,
            d.allow_unknown, d.max_goals) == (2, 0.0, 1, 1, 8, 16, 64, 20, 10, 1, 256)
    # the tsdf defaults for the geometry
    tc = _lib.TsdfConfig()
    L.aria_tsdf_default_config(C.byref(tc))
    assert (tc.nx, tc.ny, tc.nz, tc.voxel, tuple(tc.origin), tc.min_weight) == (cfg.nx, cfg.ny, cfg.nz, cfg.voxel, tuple(cfg.origin), cfg.min_weight)
    assert L.aria_nav_field_bytes(256, 128, 256) == 32 << 20 == R.field_bytes(256, 128, 256)
    assert L.aria_nav_field_bytes(12, 8, 1) == -1 and L.aria_nav_field_bytes(8, 8, 0) == -1 and L.aria_nav_field_bytes(8, 1032, 1) == -1
    assert L.aria_nav_check(None) == -1 and L.aria_nav_solve_device(None, None, 0) == -1
    assert R.default_band(8) == (0, 8) and R.default_band(64) == (24, 48)


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("nx", 12), ("ny", 0), ("nz", 1032), ("up_axis", 3), ("up_axis", -1),
                                         ("band0", -1), ("band0", 144), ("band1", 257), ("min_weight", 0), ("min_weight", 65536),
                                         ("occ_tsdf", float("nan")), ("occ_count", 0), ("free_count", 0), ("clear_radius", -1),
                                         ("clear_radius", 65), ("block_d2", -1), ("block_d2", 65), ("soft_d2", 0), ("soft_d2", 82),
                                         ("penalty", -1), ("penalty", 1001), ("unknown_penalty", 1001), ("allow_unknown", 2),
                                         ("max_goals", 0), ("max_goals", 65536), ("voxel", 0.0), ("voxel", float("inf"))])
def test_nav_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched, and the restatement refuses the same."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.NavConfig()
    L.aria_nav_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_nav_create(C.byref(cfg), C.byref(h)) == -1        # ARIA_E_INVALID
    assert not h.value
    assert L.aria_nav_create(None, C.byref(h)) == -1
    if field == "struct_size":
        return
    kw = {field: value}
    if field in ("nx", "ny", "nz"):
        dims = {"nx": 256, "ny": 256, "nz": 128}
        dims[field] = value
        kw = dict(dims=(dims["nx"], dims["ny"], dims["nz"]))
    elif field in ("band0", "band1"):
        band = {"band0": 120, "band1": 144}
        band[field] = value
        kw = dict(band=(band["band0"], band["band1"]))
    with pytest.raises(ValueError):
        R.config(**kw)


def test_hand_made_grid_known_answers():
    """The 8 x 8 grid of nav_cases.HAND_ROWS under R = 1, block_d2 = 1, soft_d2 = 4, penalty = 7, unknown_penalty = 3, goal (7, 0):
    clearance, costs, the field and one path, written out. pen = 7*(4 - d2)/4: 5 beside an obstacle, 3 diagonally off one."""
    case = NC.hand()
    assert case.d2.tolist() == [[4, 2, 1, 2, 4, 4, 4, 4],
                                [4, 1, 0, 1, 4, 4, 4, 4],
                                [4, 1, 0, 1, 1, 1, 2, 4],
                                [4, 1, 0, 0, 0, 0, 1, 4],
                                [2, 1, 1, 1, 1, 1, 2, 4],
                                [1, 0, 1, 4, 4, 4, 4, 4],
                                [2, 1, 2, 4, 4, 2, 1, 2],
                                [4, 4, 4, 4, 4, 1, 0, 1]]
    assert case.cost.tolist() == [[0, 3, 5, 3, 0, 0, 0, 0],
                                  [0, 5, B, 5, 0, 0, 0, 0],
                                  [0, 5, B, 5, 5, 8, 3, 0],          # (5, 2) is UNKNOWN: 5 + 3
                                  [0, 5, B, B, B, B, 5, 0],
                                  [3, 5, 5, 5, 5, 5, 3, 0],
                                  [5, B, 5, 0, 0, 0, 0, 0],
                                  [3, 5, 3, 0, 0, 3, 5, 3],
                                  [0, 0, 0, 0, 0, 5, B, 5]]
    # along the top row towards the goal every step is 10 + pen of the cell stepped on: 10, 20, 30, 40, 53, 68, 81
    assert case.fields[0].tolist() == [[81, 68, 53, 40, 30, 20, 10, 0],
                                       [85, 81, I, 44, 34, 24, 14, 10],
                                       [95, 96, I, 48, 38, 28, 24, 20],
                                       [105, 109, I, I, I, I, 34, 30],
                                       [115, 110, 95, 85, 72, 57, 44, 40],
                                       [128, I, 91, 81, 71, 61, 54, 50],
                                       [123, 108, 95, 85, 75, 68, 64, 60],
                                       [119, 109, 99, 89, 85, 81, I, 73]]
    rec, paths, truncated = R.trace(case.cost, case.d2, case.fields, case.goals, case.queries, 16)
    assert not truncated
    # from (0, 7): east along the bottom row, then north-east under the wall, then north along the free right-hand column
    assert rec[0].tolist() == (119, 11, 2, R.OK) and paths[0, :11].tolist() == [56, 57, 58, 59, 52, 45, 38, 31, 23, 15, 7]
    # from (3, 2) the diagonal to (4, 1) is allowed, the one from (3, 1) to (2, 0) would cut the corner of (2, 1)
    assert rec[1].tolist() == (48, 5, 1, R.OK) and paths[1, :5].tolist() == [19, 12, 13, 14, 7]
    assert rec[2].tolist() == (I, 0, 0, R.UNREACHABLE)               # a start on an obstacle
    assert not R.allowed_moves(case.cost)[1, 3] >> 7 & 1             # (3, 1) -> (2, 0): refused by the corner rule
    # truncation keeps the totals
    rec2, paths2, truncated = R.trace(case.cost, case.d2, case.fields, case.goals, case.queries, 4, np.full((3, 4), -7, np.int32))
    assert truncated and rec2[0].tolist() == (119, 11, 2, R.TRUNCATED) and paths2[0].tolist() == [56, 57, 58, 59]
    assert rec2[2].tolist() == rec[2].tolist() and paths2[2].tolist() == [-7] * 4


@pytest.mark.parametrize("name", ["hand", "random8", "random24x16", "empty", "many", "clear8"])
def test_dijkstra_equals_the_fixed_point_sweeps(name):
    case = {"hand": NC.hand, "random8": lambda: NC.random_grid(8, 8), "random24x16": lambda: NC.random_grid(24, 16), "empty": NC.empty,
            "many": NC.many, "clear8": lambda: NC.clearance_case(8, 1)}[name]()
    for g, want in list(zip(case.goals, case.fields))[:16]:
        got, sweeps = R.field_sweeps(case.cost, g)
        assert got.tobytes() == want.tobytes(), (name, g)
        assert sweeps >= 1 or not (want != R.INF).any()
    # a goal that is blocked or outside the grid: all INF, by both
    for g in ((-1, 0), (0, case.cost.shape[0])) + tuple(map(tuple, np.argwhere(case.cost == B)[:1, ::-1])):
        assert (R.field(case.cost, g) == I).all() and (R.field_sweeps(case.cost, g)[0] == I).all()


def test_cells_from_a_hand_built_volume():
    """Rule 2: the band edges are included and excluded exactly, a weight one below min_weight is ignored, tsdf == occ_tsdf is not
    solid, a NaN is not solid, and OCCUPIED wins over FREE."""
    cfg, vol, want = NC.hand_volume()
    got = R.cells_from_volume(vol, cfg)
    assert got.tolist() == want.tolist()
    assert (got == R.OCCUPIED).sum() == 2 and (got == R.FREE).sum() == 4
    # the same columns under the other up axes: the volume turned so that the band axis is x, then z
    for up, axes in ((0, (0, 2, 1)), (2, (1, 0, 2))):
        c2 = R.config(dims=(8, 8, 8), up_axis=up, band=cfg.band, min_weight=cfg.min_weight, occ_tsdf=cfg.occ_tsdf, occ_count=2, free_count=2,
                      clear_radius=1, block_d2=1, soft_d2=4)
        turned = np.ascontiguousarray(vol.transpose(axes))
        got2 = R.cells_from_volume(turned, c2)
        assert got2.tolist() == want.tolist(), up                     # (U, V) is again (old x, old z)
    with pytest.raises(ValueError):
        R.check_cells(np.full((8, 8), 3, np.uint8), cfg)
    with pytest.raises(ValueError):
        R.check_cells(np.zeros((8, 4), np.uint8), cfg)


def test_world_helpers():
    cfg = R.config(dims=(32, 24, 16), up_axis=1, band=(10, 14), voxel=0.1, origin=(-1.6, -1.2, 1.2))
    X = np.array([[-1.6, 0.0, 1.2], [1.59, 0.3, 2.79], [0.05, -5.0, 2.05], [-1.61, 0.0, 2.81]], f32)
    assert R.cell_of(X, cfg).tolist() == [[0, 0], [31, 15], [16, 8], [-1, 16]]
    c = R.centre_of([[0, 0], [31, 15]], cfg)
    assert c.dtype == f32 and c[0].tolist() == [f32(-1.6) + f32(0.5) * f32(0.1), f32(-1.2) + f32(12.0) * f32(0.1), f32(1.2) + f32(0.5) * f32(0.1)]
    assert R.cell_of(c, cfg).tolist() == [[0, 0], [31, 15]]
    assert R.plane_axes(0) == (1, 2) and R.plane_axes(1) == (0, 2) and R.plane_axes(2) == (0, 1)


def test_case_conditions():
    """What the device tests rely on, asserted on the restatement."""
    for nu, nv in ((8, 8), (24, 16)):
        case = NC.random_grid(nu, nv)
        rec, paths, _ = NC.traced("random%dx%d" % (nu, nv), case, 64, NC.GUARD32)
        assert (rec["status"] == R.OK).any() and (rec["status"] == R.UNREACHABLE).any() and (rec["status"] == R.OUT_OF_GRID).sum() == 3
        diag = sum(int((np.abs(NC.path_moves(p[:n], nu)).sum(axis=1) == 2).sum()) for p, n in zip(paths, rec["n_cells"]) if n > 1)
        assert diag > 0 and NC.refused_diagonals(case.cost) > 0
    s = NC.serpentine()
    rec = NC.traced("serpentine", s, 2100, NC.GUARD32)[0]
    assert rec["n_cells"][0] >= 1000 and rec["n_cells"][1] >= 1000 and rec["status"][3] == R.UNREACHABLE
    for radius in (1, 8):
        for au in (0, 1):
            c = NC.clearance_case(radius, au)
            by_clearance = (c.cells == R.FREE) & (c.cost == B)
            penalised = (c.cells == R.FREE) & (c.cost != B) & (c.cost > 0)
            assert by_clearance.any() and penalised.any()
            unknown = c.cost[c.cells == R.UNKNOWN]
            assert (unknown == B).all() if au == 0 else (unknown != B).any()
            assert c.d2[NC.PROBE[1], NC.PROBE[0]] == radius * radius       # the obstacle at R counts, the one at R + 1 does not
    assert NC.clearance_case(0, 1).d2[NC.PROBE[1], NC.PROBE[0]] == 1
    for up in (0, 1, 2):
        case, _ = NC.chain(up)
        assert all((case.cells == s).any() for s in (R.FREE, R.OCCUPIED, R.UNKNOWN))
        rec = NC.traced("chain%d" % up, case, 64, NC.GUARD32)[0]
        assert (rec["status"] == R.OK).sum() >= 5
