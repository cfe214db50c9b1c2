"""Path planning on the MI355X (aria_nav_*, kernels in aria_slam_amd/csrc/nav_grid.hip) against its definition, the NumPy
restatement aria_slam_amd/nav_ref.py: cells, clearance, costs, fields, records and paths are BITWISE equal. The stage is
integer arithmetic and rule 6 has one least solution, so a difference is a bug, never a tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nav_cases as NC   # noqa: E402
from aria_slam_amd import nav_ref as R   # noqa: E402

ARIA_E_INVALID, ARIA_E_NO_DEVICE, ARIA_E_OUTPUT_TOO_SMALL = -1, -2, -5
_KW = ("up_axis", "band", "min_weight", "occ_tsdf", "occ_count", "free_count", "clear_radius", "block_d2", "soft_d2", "penalty",
       "unknown_penalty", "allow_unknown", "max_goals", "voxel", "origin")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def work(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return s


def _dev(torch, work, a):
    with torch.cuda.stream(work):
        t = torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to("cuda:0")       # a copy: the shared cases are read-only
    work.synchronize()
    return t


def _full(torch, work, nbytes, value):
    with torch.cuda.stream(work):
        t = torch.full((max(nbytes, 1),), value, dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _handle(aria, work, cfg):
    return aria.HipPathPlanner(dims=cfg.dims, stream=work.cuda_stream, **{k: getattr(cfg, k) for k in _KW})


def _check_grid(h, case, what):
    for name, got, want in (("cells", h.cells(), case.cells), ("clearance", h.clearance(), case.d2), ("costs", h.costs(), case.cost)):
        print("%s %s: %d of %d differ" % (what, name, int((got != want).sum()), want.size))
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, name)


def _check_plan(torch, work, h, case, name, path_cap, want_status=0):
    """solve_device + trace_device with guard patterns beyond the records, the paths and Q; fields, records and paths bitwise."""
    G, Q = len(case.goals), len(case.queries)
    want_rec, want_paths, trunc = NC.traced(name, case, path_cap, NC.GUARD32)
    h.solve_device(_dev(torch, work, case.goals), G)
    d_rec = _full(torch, work, 16 * (Q + 2), NC.GUARD)
    d_paths = _full(torch, work, 4 * (Q * path_cap + 8), NC.GUARD)
    h.trace_device(_dev(torch, work, case.queries), Q, d_rec, d_paths, path_cap)
    status = h.status()
    for g in range(G):
        got = h.field(g)
        if got.tobytes() != case.fields[g].tobytes():
            print("%s field %d: %d of %d cells differ" % (name, g, int((got != case.fields[g]).sum()), got.size))
        assert got.tobytes() == case.fields[g].tobytes(), (name, "field", g)
    rec = d_rec.cpu().numpy().view(R.RECORD_DTYPE)
    paths = d_paths.cpu().numpy().view(np.int32)
    print("%s: G %d Q %d, status counts %s, rounds %s" % (name, G, Q, np.bincount(want_rec["status"], minlength=4).tolist(),
                                                           h.rounds(G)[:8].tolist()))
    assert rec[:Q].tobytes() == want_rec.tobytes(), (name, rec[:Q], want_rec)
    assert (rec[Q:].view(np.uint8) == NC.GUARD).all()
    assert paths[:Q * path_cap].tobytes() == want_paths.tobytes(), name
    assert (paths[Q * path_cap:] == NC.GUARD32).all()
    assert status == (ARIA_E_OUTPUT_TOO_SMALL if trunc else 0) == want_status and h.status() == 0      # deferred, reported once
    return rec[:Q], paths[:Q * path_cap].reshape(Q, path_cap)


def _run_case(aria, torch, work, case, name, path_cap, want_status=0):
    h = _handle(aria, work, case.cfg)
    try:
        h.set_cells_device(_dev(torch, work, case.cells))
        assert h.status() == 0
        _check_grid(h, case, name)
        return _check_plan(torch, work, h, case, name, path_cap, want_status)
    finally:
        h.close()


@pytest.mark.parametrize("nu,nv", [(8, 8), (24, 16)])
def test_random_obstacles_equal_the_restatement(aria, torch_cuda, work, nu, nv):
    """The smallest grid and one with nu != nv (a swapped index shows): about 25 % obstacles, G = 5, Q = 40. On the restatement:
    statuses 0 and 1 both occur, some path takes a diagonal, and the corner rule refuses some diagonal."""
    case = NC.random_grid(nu, nv)
    assert len(case.goals) == 5 and len(case.queries) == 40
    rec, paths = _run_case(aria, torch_cuda, work, case, "random%dx%d" % (nu, nv), 64)
    assert (rec["status"] == R.OK).any() and (rec["status"] == R.UNREACHABLE).any() and (rec["status"] == R.OUT_OF_GRID).any()
    diag = sum(int((np.abs(NC.path_moves(p[:n], nu)).sum(axis=1) == 2).sum()) for p, n in zip(paths, rec["n_cells"]) if n > 1)
    assert diag > 0 and NC.refused_diagonals(case.cost) > 0


def test_empty_grid_only_the_move_order_decides(aria, torch_cuda, work):
    """16 x 16 without obstacles and penalty = 0: every path has many equal-cost alternatives."""
    case = NC.empty()
    assert case.cfg.penalty == 0 and not case.cost.any()
    rec, _ = _run_case(aria, torch_cuda, work, case, "empty", 32)
    assert (rec["status"] == R.OK).all()


def test_serpentine_settles_and_truncation_keeps_the_totals(aria, torch_cuda, work):
    """64 x 64 with walls that leave one corridor: the start-to-goal path has at least 1000 cells, far more than one sweep
    propagates, so a relaxation that stops early shows. With path_cap = 100 the long queries are TRUNCATED, the totals are
    intact, the guard survives beyond the cap and beyond Q, and ARIA_E_OUTPUT_TOO_SMALL is reported once."""
    torch = torch_cuda
    case = NC.serpentine()
    full = NC.traced("serpentine", case, 2100, NC.GUARD32)[0]
    assert full["n_cells"][0] >= 1000 and full["n_cells"][1] >= 1000
    h = _handle(aria, work, case.cfg)
    try:
        h.set_cells(case.cells)                                      # the host form
        _check_grid(h, case, "serpentine")
        _check_plan(torch, work, h, case, "serpentine", 2100)
        rec, paths = _check_plan(torch, work, h, case, "serpentine", 100, ARIA_E_OUTPUT_TOO_SMALL)
        assert rec["status"].tolist() == [R.TRUNCATED, R.TRUNCATED, R.TRUNCATED, R.UNREACHABLE]
        assert rec["n_cells"].tolist() == full["n_cells"].tolist() and rec["cost"].tolist() == full["cost"].tolist()
        # the host form of solve + trace: the same, and what it does not write keeps the caller's bytes
        got_rec, got_paths, trunc = h.plan(case.goals, case.queries, 100, paths=np.full((4, 100), NC.GUARD32, np.int32))
        assert trunc and got_rec.tobytes() == rec.tobytes() and got_paths.tobytes() == paths.tobytes()
        assert h.status() == 0
    finally:
        h.close()


@pytest.mark.parametrize("radius", [0, 1, 8])
@pytest.mark.parametrize("allow_unknown", [0, 1])
def test_clearance_and_penalties(aria, torch_cuda, work, radius, allow_unknown):
    """32 x 32 with obstacles on the border, in the corners and at distance exactly R (inside the window) and R + 1 (outside it)
    from the probe cell. For R = 1 and 8 cells blocked by clearance alone and penalised cells both exist. (For R = 0 neither
    can: a cell that is not OCCUPIED has d2 = CAP = 1 there, and block_d2 <= soft_d2 <= CAP.)"""
    case = NC.clearance_case(radius, allow_unknown)
    free = case.cells == R.FREE
    if radius > 0:
        assert (free & (case.cost == R.BLOCKED)).any() and (free & (case.cost != R.BLOCKED) & (case.cost > 0)).any()
    assert case.d2[NC.PROBE[1], NC.PROBE[0]] == max(radius * radius, 1)
    unknown = case.cost[case.cells == R.UNKNOWN]
    assert (unknown == R.BLOCKED).all() if allow_unknown == 0 else (unknown != R.BLOCKED).any()
    _run_case(aria, torch_cuda, work, case, "clear_%d_%d" % (radius, allow_unknown), 64)


def test_field_storage_beyond_lds(aria, torch_cuda, work):
    """256 x 256: 256 KiB of int32 cannot sit in the 160 KiB of a CU's LDS, so the fields are relaxed where they lie in HBM."""
    case = NC.big()
    assert 4 * case.cost.size > 160 * 1024 and len(case.goals) == 4
    rec, _ = _run_case(aria, torch_cuda, work, case, "big", 512)
    assert (rec["status"] == R.OK).all() and rec["n_cells"].max() > 256


def test_default_plane_in_lds_above_64_kib(aria, torch_cuda, work):
    """256 x 128 under the default radii: the field of a goal takes 131 584 B of LDS, more than the 64 KiB a kernel gets without
    asking. A second, small handle is alive and created AFTER the large one: the LDS limit of the field kernel belongs to the
    function, and a later handle must not lower it under an earlier one."""
    torch = torch_cuda
    case = NC.default_plane()
    small = NC.hand()
    h = _handle(aria, work, case.cfg)
    h2 = _handle(aria, work, small.cfg)
    try:
        h.set_cells(case.cells)
        h2.set_cells(small.cells)
        _check_plan(torch, work, h2, small, "hand", 16)
        _check_grid(h, case, "default plane")
        rec, _ = _check_plan(torch, work, h, case, "default_plane", 512)
        assert rec["status"][0] == R.OK and rec["n_cells"][0] > 256 and rec["status"][1] == R.OK
        assert (rec["status"] == R.UNREACHABLE).any()                # the closed room
    finally:
        h.close()
        h2.close()


def test_many_goals(aria, torch_cuda, work):
    """16 x 16 with max_goals = G = 320, more goals than the card has CUs: a duplicate goal, a goal on a blocked cell, a goal
    outside the grid, a goal that is its own start. G = 321 is refused; G = 0 and Q = 0 are accepted."""
    torch = torch_cuda
    case = NC.many()
    assert len(case.goals) == NC.N_MANY == case.cfg.max_goals
    assert case.fields[7].tobytes() == case.fields[3].tobytes() and (case.fields[11] == R.INF).all() and (case.fields[13] == R.INF).all()
    h = _handle(aria, work, case.cfg)
    try:
        h.set_cells(case.cells)
        rec, paths = _check_plan(torch, work, h, case, "many", 40)
        assert rec["status"][:4].tolist() == [R.OK, R.UNREACHABLE, R.OUT_OF_GRID, R.OK]
        assert rec[3].tolist() == (0, 1, int(case.d2[case.goals[319][1], case.goals[319][0]]), R.OK)
        L = aria.load_library()
        d_g = _dev(torch, work, np.concatenate([case.goals, case.goals[:1]]))
        assert L.aria_nav_solve_device(h._h, d_g.data_ptr(), NC.N_MANY + 1) == ARIA_E_INVALID
        d_rec = _full(torch, work, 16, NC.GUARD)
        h.trace_device(None, 0, None, None, 0)                       # Q = 0 against the fields that are there
        h.solve_device(None, 0)                                      # G = 0: accepted; every goal index is now outside [0, G)
        h.trace_device(_dev(torch, work, np.array([[1, 1, 0]], np.int32)), 1, d_rec, None, 0)
        assert h.status() == 0
        assert d_rec.cpu().numpy().view(R.RECORD_DTYPE)[0].tolist() == (R.INF, 0, 0, R.OUT_OF_GRID)
        rec0, paths0, trunc = h.plan(np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32), 8)
        assert len(rec0) == 0 and paths0.shape == (0, 8) and not trunc
    finally:
        h.close()


@pytest.mark.parametrize("up_axis", [0, 1, 2])
def test_chain_volume_to_paths(aria, torch_cuda, work, up_axis):
    """tsdf_cases.ref_scene() integrated on the device, its device_voxels() handed to aria_nav_update_from_volume_device on the
    same stream, a plan across the scene: cells, clearance, costs, fields, records and paths equal tsdf_ref followed by
    nav_ref. The band cuts the sphere; all three cell states occur."""
    import tsdf_cases as TC
    torch = torch_cuda
    case, _ = NC.chain(up_axis)
    assert all((case.cells == s).any() for s in (R.FREE, R.OCCUPIED, R.UNKNOWN))
    tcfg = TC.scene_config()
    d, im, e = TC.scene_frames()
    vol = aria.HipTsdfVolume(dims=tcfg.dims, voxel=tcfg.voxel, origin=tcfg.origin, trunc=tcfg.trunc, min_depth=tcfg.min_depth,
                             max_depth=tcfg.max_depth, max_weight=tcfg.max_weight, min_weight=tcfg.min_weight, K=tcfg.K,
                             stream=work.cuda_stream)
    h = None
    try:
        vol.integrate_batch_device(_dev(torch, work, d), TC.W, TC.H, _dev(torch, work, e), 3, None, _dev(torch, work, im))
        h = aria.HipPathPlanner.from_volume(vol, stream=work.cuda_stream, up_axis=up_axis, band=NC.CHAIN_BANDS[up_axis],
                                            **{k: getattr(case.cfg, k) for k in ("clear_radius", "block_d2", "soft_d2", "penalty", "unknown_penalty")})
        assert h.ref_config == case.cfg
        h.update(vol)                                                # the same stream: ordered after the integration
        assert vol.status() == 0 and h.status() == 0
        _check_grid(h, case, "chain %d" % up_axis)
        rec, _ = _check_plan(torch, work, h, case, "chain%d" % up_axis, 64)
        assert rec["status"][0] == R.OK and rec["n_cells"][0] > 8
        # the world helpers agree with the restatement's
        assert h.cell_of(h.centre_of(case.goals)).tolist() == case.goals.tolist()
    finally:
        if h is not None:
            h.close()
        vol.close()


def test_lifecycle_and_refusals(aria, torch_cuda, work):
    """Create refuses a bad struct size and a device that is not there; a borrowed stream is reported and survives close; a
    second close is a no-op; NULL pointers and negative counts are refused before anything is enqueued; a trace before a solve
    and a trace after set_cells without a new solve are refused; a cell value of 3 is refused by the host form and deferred by
    the device form, and the old cells stay."""
    from aria_slam_amd import _lib
    torch = torch_cuda
    L = aria.load_library()
    cfg = _lib.NavConfig()
    L.aria_nav_default_config(C.byref(cfg))
    hh = C.c_void_p()
    cfg.struct_size += 4
    assert L.aria_nav_create(C.byref(cfg), C.byref(hh)) == ARIA_E_INVALID and not hh.value
    cfg.struct_size -= 4
    cfg.device = torch.cuda.device_count()
    assert L.aria_nav_create(C.byref(cfg), C.byref(hh)) == ARIA_E_NO_DEVICE and not hh.value
    assert ("device %d not present" % cfg.device) in L.aria_last_hip_error().decode()

    case = NC.hand()
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    kw = {k: getattr(case.cfg, k) for k in _KW}
    h = aria.HipPathPlanner(dims=case.cfg.dims, stream=s.cuda_stream, **kw)
    own = aria.HipPathPlanner(dims=case.cfg.dims, **kw)
    try:
        assert h.stream == s.cuda_stream and own.stream and own.stream != s.cuda_stream
        for x in (h, own):
            assert x.status() == 0 and (x.cells() == R.UNKNOWN).all() and x.device_fields()       # a new handle: UNKNOWN cells
            x.check()
        d_g = _dev(torch, work, case.goals)
        d_q = _dev(torch, work, case.queries)
        d_rec = _full(torch, work, 16 * 3, NC.GUARD)
        d_paths = _full(torch, work, 4 * 3 * 16, NC.GUARD)
        trace = lambda **k: L.aria_nav_trace_device(   # noqa: E731
            h._h, k.get("q", d_q.data_ptr()), k.get("n", 3), k.get("rec", d_rec.data_ptr()), k.get("paths", d_paths.data_ptr()), k.get("cap", 16))
        assert trace() == ARIA_E_INVALID                             # a trace before a solve
        assert L.aria_nav_read_field(h._h, 0, np.zeros(64, np.int32).ctypes.data) == ARIA_E_INVALID
        h.set_cells(case.cells)
        assert trace() == ARIA_E_INVALID
        assert L.aria_nav_solve_device(h._h, None, 1) == ARIA_E_INVALID and L.aria_nav_solve_device(h._h, d_g.data_ptr(), -1) == ARIA_E_INVALID
        assert L.aria_nav_solve_device(h._h, d_g.data_ptr(), 1) == 0 and trace() == 0
        for k in (dict(q=None), dict(rec=None), dict(paths=None), dict(n=-1), dict(cap=-1)):
            assert trace(**k) == ARIA_E_INVALID, k
        assert trace(paths=None, cap=0) == 0 and h.status() == ARIA_E_OUTPUT_TOO_SMALL and h.status() == 0
        assert L.aria_nav_read_field(h._h, 1, np.zeros(64, np.int32).ctypes.data) == ARIA_E_INVALID       # one goal only
        assert L.aria_nav_set_cells_device(h._h, None) == ARIA_E_INVALID and L.aria_nav_set_cells(h._h, None) == ARIA_E_INVALID
        assert L.aria_nav_update_from_volume_device(h._h, None) == ARIA_E_INVALID
        assert L.aria_nav_read_cells(h._h, None) == ARIA_E_INVALID and L.aria_nav_read_costs(None, None) == ARIA_E_INVALID
        assert L.aria_nav_plan(h._h, None, 1, None, 0, None, None, 0) == ARIA_E_INVALID
        assert L.aria_nav_plan(h._h, None, 0, None, 1, None, None, 0) == ARIA_E_INVALID
        assert h.field(0).tobytes() == case.fields[0].tobytes()
        # a cell value of 3: the host form refuses, the device form defers; the old cells, and so the fields' map, stay
        bad = case.cells.copy()
        bad[4, 4] = 3
        with pytest.raises(aria.AriaError) as err:
            h.set_cells(bad)
        assert err.value.status == ARIA_E_INVALID and trace() == 0   # nothing changed: the fields are still this map's
        h.set_cells_device(_dev(torch, work, bad))
        assert h.status() == ARIA_E_INVALID and h.status() == 0
        _check_grid(h, case, "after a refused set_cells_device")
        assert trace() == ARIA_E_INVALID                             # a device set_cells always asks for a new solve
        h.set_cells(np.zeros((8, 8), np.uint8))                      # the map changed: a new solve is needed
        assert trace() == ARIA_E_INVALID and L.aria_nav_solve_device(h._h, d_g.data_ptr(), 1) == 0 and trace() == 0
        assert h.status() == 0
    finally:
        h.close()
        own.close()
    h.close()                                                        # a second close is a no-op
    with torch.cuda.stream(s):
        x = torch.arange(8, device="cuda:0") * 2
    s.synchronize()
    assert int(x.sum()) == 56
