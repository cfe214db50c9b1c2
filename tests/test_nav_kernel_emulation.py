"""The kernel source of aria_slam_amd/csrc/nav_grid.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/nav_ref.py) on the cases tests/test_gpu_nav.py runs on the device.

The text of the file between "namespace {" and the goal-field section -- k_nav_columns, k_nav_validate, k_nav_adopt, k_nav_span,
k_nav_clearance, k_nav_cost, k_nav_moves and k_nav_trace -- is pasted between tests/cpp/nav_kernel_emu_head.inc (a shim: the
lanes of a workgroup one after the other; these kernels have no barrier) and nav_kernel_emu_tail.inc (the parameters, the launch
geometry and the launch order) and compiled with the clang++ that hipcc drives. What this checks without a GPU is the indexing
of the three up axes, the two-pass clearance against the brute-force window, the cost and move rules and the trace; the trace
is fed the restatement's fields. What it cannot check is the field kernel (a workgroup with barriers), the device's streams and
the lifecycle: that is tests/test_gpu_nav.py.

The field kernel itself has barriers and stays on the GPU, but its relaxation, nav_relax, is plain: that text is pasted in as
well, and tests/cpp/nav_field_emu_tail.inc restates the kernel's rounds around it with the lanes of a phase one after the other.
That holds the relaxation and both schedules (row and column sweeps at either pitch, and the plain all-cell sweep of the variants
build) to the restatement, and counts their rounds under that one interleaving."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nav_cases as NC   # noqa: E402
from aria_slam_amd import nav_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "nav_grid.hip")).read()
    body = src[src.index("\nnamespace {"):src.index("\n// ---- goal fields")]
    for k in ("k_nav_columns", "k_nav_validate", "k_nav_adopt", "k_nav_span", "k_nav_clearance", "k_nav_cost", "k_nav_moves", "k_nav_trace"):
        assert k in body, k
    assert "asm" not in body and "__shared__" not in body and "__syncthreads" not in body, "plain HIP C++, no LDS, no barrier"
    relax = src[src.index("\ntemplate <typename Ptr>\n"):src.index("\ntemplate <bool LDS>")]
    assert "nav_relax" in relax and "__shared__" not in relax and "__syncthreads" not in relax
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("nav_kernel_emu_head.inc", "nav_kernel_emu_tail.inc",
                                                                            "nav_field_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "nav_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "nav_emu.cpp"), os.path.join(out_dir, "libnav_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + relax + parts[1] + parts[2])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-fPIC", "-shared", "-w", "-I", os.path.join(ROOT, "include"), "-o", so, cpp])
    L = C.CDLL(so)
    p, i = C.c_void_p, C.c_int
    L.emu_columns.argtypes = [p, C.c_float, p, p]
    L.emu_columns.restype = None
    L.emu_set_cells.argtypes = [p, p, p, p]
    L.emu_rebuild.argtypes = [p, p, p, p, p, p]
    L.emu_rebuild.restype = None
    L.emu_trace.argtypes = [i, i, p, p, p, p, i, p, i, p, p, i, p]
    L.emu_trace.restype = None
    L.emu_field.argtypes = [i, i, p, i, i, p, i, i, i]
    return L


def _ip(cfg):
    return np.array([*cfg.dims, cfg.up_axis, *cfg.band, cfg.min_weight, cfg.occ_count, cfg.free_count, cfg.clear_radius, cfg.block_d2,
                     cfg.soft_d2, cfg.penalty, cfg.unknown_penalty, cfg.allow_unknown], np.int32)


def _rebuild(L, cfg, cells):
    nu, nv = R.grid_shape(cfg)
    cells = np.ascontiguousarray(cells, np.uint8)
    span, d2, cost, cm = (np.zeros((nv, nu), t) for t in (np.uint8, np.uint16, np.uint16, np.uint32))
    ip = _ip(cfg)
    L.emu_rebuild(ip.ctypes.data, cells.ctypes.data, span.ctypes.data, d2.ctypes.data, cost.ctypes.data, cm.ctypes.data)
    return d2, cost, cm


def _trace(L, case, cm, path_cap, fill=NC.GUARD32):
    nu, nv = R.grid_shape(case.cfg)
    Q = len(case.queries)
    rec = np.zeros(Q + 2, R.RECORD_DTYPE)
    rec.view(np.uint8)[:] = NC.GUARD
    paths = np.full((Q + 1, max(path_cap, 1)), fill, np.int32)
    err = np.zeros(1, np.int32)
    fields, goals, queries, d2 = (np.ascontiguousarray(a) for a in (case.fields, case.goals, case.queries, case.d2))
    L.emu_trace(nu, nv, cm.ctypes.data, d2.ctypes.data, fields.ctypes.data, goals.ctypes.data, len(goals), queries.ctypes.data, Q,
                rec.ctypes.data, paths.ctypes.data, path_cap, err.ctypes.data)
    assert (rec[Q:].view(np.uint8) == NC.GUARD).all(), "records beyond Q were touched"
    return rec[:Q], paths.reshape(-1)[:Q * path_cap].reshape(Q, path_cap), paths.reshape(-1)[Q * path_cap:], int(err[0])


def _check_case(L, name, case, path_cap):
    d2, cost, cm = _rebuild(L, case.cfg, case.cells)
    assert d2.tobytes() == case.d2.tobytes(), (name, int((d2 != case.d2).sum()))
    assert cost.tobytes() == case.cost.tobytes(), (name, int((cost != case.cost).sum()))
    want_cm = case.cost.astype(np.uint32) | (R.allowed_moves(case.cost).astype(np.uint32) << 16)
    assert cm.tobytes() == want_cm.tobytes(), name
    want_rec, want_paths, trunc = NC.traced(name, case, path_cap, NC.GUARD32)
    rec, paths, beyond, err = _trace(L, case, cm, path_cap)
    assert rec.tobytes() == want_rec.tobytes(), (name, rec, want_rec)
    assert paths.tobytes() == want_paths.tobytes(), name
    assert (beyond == NC.GUARD32).all()
    assert err == (4 if trunc else 0)                                # ERRBIT_NAV_CAP alone


@pytest.mark.parametrize("name", ["hand", "random8", "random24x16", "empty", "serpentine", "many"])
def test_grid_kernels_and_trace_are_bitwise_the_restatement(emu, name):
    case, cap = {"hand": (NC.hand, 16), "random8": (lambda: NC.random_grid(8, 8), 64), "random24x16": (lambda: NC.random_grid(24, 16), 64),
                 "empty": (NC.empty, 32), "serpentine": (NC.serpentine, 2100), "many": (NC.many, 40)}[name]
    _check_case(emu, name, case(), cap)


def test_trace_truncates_and_touches_nothing_beyond(emu):
    """The serpentine with path_cap = 100: status 3, the totals intact, the cells beyond the cap and beyond Q untouched."""
    case = NC.serpentine()
    _check_case(emu, "serpentine", case, 100)
    rec = NC.traced("serpentine", case, 100, NC.GUARD32)[0]
    assert (rec["status"] == R.TRUNCATED).any() and rec["n_cells"].max() >= 1000
    _check_case(emu, "serpentine", case, 0)                          # path_cap = 0: the records alone


@pytest.mark.parametrize("radius", [0, 1, 8])
@pytest.mark.parametrize("allow_unknown", [0, 1])
def test_two_pass_clearance_is_the_brute_force_window(emu, radius, allow_unknown):
    _check_case(emu, "clear_%d_%d" % (radius, allow_unknown), NC.clearance_case(radius, allow_unknown), 64)


def test_clearance_of_random_cells_at_every_radius_class(emu):
    """Random grids of 40 x 24 under R = 0, 1, 2, 5, 13, 64 (a window larger than the grid)."""
    rng = np.random.default_rng(3)
    for radius in (0, 1, 2, 5, 13, 64):
        cfg = NC.grid_config(40, 24, clear_radius=radius, block_d2=min(2, (radius + 1) ** 2), soft_d2=(radius + 1) ** 2, penalty=1000)
        cells = (rng.random((24, 40)) < 0.04).astype(np.uint8) + 2 * (rng.random((24, 40)) < 0.1).astype(np.uint8)
        cells[cells == 3] = 1
        d2, cost, _ = _rebuild(emu, cfg, cells)
        want_d2, want_cost = R.build(cells, cfg)
        assert d2.tobytes() == want_d2.tobytes() and cost.tobytes() == want_cost.tobytes(), radius


def test_columns_kernel_on_the_hand_built_volume_and_the_scene(emu):
    """Rule 2: the band edges, weight one below min_weight, tsdf == occ_tsdf; then the TSDF scene under each up axis."""
    cfg, vol, want = NC.hand_volume()
    cases = [(cfg, vol, want)]
    for up in (0, 1, 2):
        case, svol = NC.chain(up)
        cases.append((case.cfg, svol, case.cells))
    for cfg, vol, want in cases:
        nu, nv = R.grid_shape(cfg)
        got = np.full((nv, nu), NC.GUARD, np.uint8)
        ip = _ip(cfg)
        v = np.ascontiguousarray(vol)
        emu.emu_columns(ip.ctypes.data, float(cfg.occ_tsdf), v.ctypes.data, got.ctypes.data)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (cfg.up_axis, int((got != want).sum()))


def test_set_cells_kernels_refuse_a_value_above_two(emu):
    cfg = NC.grid_config(8, 8)
    old = NC.hand().cells.copy()
    new = np.zeros((8, 8), np.uint8)
    new[3, 4] = 3
    err = np.zeros(1, np.int32)
    ip = _ip(cfg)
    assert emu.emu_set_cells(ip.ctypes.data, new.ctypes.data, old.ctypes.data, err.ctypes.data) == 1 and err[0] == 1
    assert old.tobytes() == NC.hand().cells.tobytes()
    new[3, 4] = 2
    err[0] = 0
    assert emu.emu_set_cells(ip.ctypes.data, new.ctypes.data, old.ctypes.data, err.ctypes.data) == 0 and err[0] == 0
    assert old.tobytes() == new.tobytes()


def _fields(L, case, lds, plain):
    nv, nu = case.cost.shape
    cm = np.ascontiguousarray(case.cost.astype(np.uint32) | (R.allowed_moves(case.cost).astype(np.uint32) << 16))
    rounds = []
    for g, want in zip(case.goals[:6], case.fields[:6]):
        D = np.full((nv, nu), NC.GUARD32, np.int32)
        r = L.emu_field(nu, nv, cm.ctypes.data, int(g[0]), int(g[1]), D.ctypes.data, lds, plain, nu * nv + 1)
        assert r >= 0, "the bound of nu*nv + 1 rounds was reached"
        assert D.tobytes() == want.tobytes(), (g, int((D != want).sum()))
        rounds.append(r)
    return rounds


@pytest.mark.parametrize("name", ["hand", "random8", "random24x16", "empty", "serpentine", "many", "clear8", "default_plane"])
def test_relaxation_schedules_reach_the_restatements_fields(emu, name):
    """nav_relax under the kernel's rounds: row and column sweeps at the LDS pitch and at the HBM pitch, and the plain all-cell
    sweep, each settle inside the bound on exactly the restatement's field, blocked and outside goals included."""
    case = {"hand": NC.hand, "random8": lambda: NC.random_grid(8, 8), "random24x16": lambda: NC.random_grid(24, 16), "empty": NC.empty,
            "serpentine": NC.serpentine, "many": NC.many, "clear8": lambda: NC.clearance_case(8, 0), "default_plane": NC.default_plane}[name]()
    sweeps = _fields(emu, case, 1, 0)
    assert _fields(emu, case, 0, 0) == sweeps                        # the pitch changes no value and no round
    plain = _fields(emu, case, 0, 1)
    print(name, "rounds, sweeps", sweeps, "plain", plain)
    if name == "serpentine":
        # a sweep settles a whole corridor, the plain schedule one cell of the path per round: 18 against 1 056 for the first goal
        assert sweeps[0] <= 64 and plain[0] >= 1000


def test_default_plane_grid_kernels_and_trace(emu):
    _check_case(emu, "default_plane", NC.default_plane(), 512)
