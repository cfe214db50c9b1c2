"""The kernel source of aria_slam_amd/csrc/icp_track.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/icp_ref.py) on every case of tests/icp_cases.py, with the shipped schedule and the plain one.

The text of the file between "namespace {" and the C-ABI section -- k_icp_prepare, k_icp_set, k_icp_accumulate, k_icp_export,
k_icp_solve and their device functions -- is pasted between tests/cpp/icp_kernel_emu_head.inc (a shim: the lanes of a wave one
after the other, the integer atomics of the wave's commit served in turn) and icp_kernel_emu_tail.inc (the parameters and
the launch geometry) and compiled with the clang++ that hipcc drives. What this checks without a GPU is the indexing, the tile
and level geometry, the order of the fp32 and fp64 operations as the host compiler takes them, the padded layouts, the
per-frame state machine (lost, level skip, masked, non-finite) and the solve; what it cannot check is the device's
arithmetic, the wave reduction and the streams: that is tests/test_gpu_icp.py.

Mutants, each put into the pasted text by hand and run once against this file (not committed):
  * the bounds test with < for <= (um < W - 1): fails every case at stride 1, odd and pitched (whose stride-4 level ends at
    column 60 = W - 1) at every stride, converged at stride 2 too; corner, fused, plane and far_map pass strides 4 and 2;
  * truncation for rintf ((float)(int) of the projected position): fails every case at every stride but odd and pitched,
    which it fails at stride 1 only, and tiny likewise;
  * the stride applied to the model lookup (ui * stride, clamped to the map): fails every case at strides 4 and 2 and, of
    course, none at stride 1, which is why test_system_* runs every level;
  * the zero-normal reject dropped: fails fused only (its 60 model hits without a normal), at every stride;
  * a partial-tile lane not masked (u < m.W dropped): passes every case of the table -- the pixel just outside a dense map
    projects outside it, and the guard bytes of `pitched` read as 1.5e16 m, no valid depth -- and fails `edge` at strides
    2 and 1 (2623 correspondences for 2537 at stride 1; at stride 4 the 16 level columns are one whole tile), which is
    why test_partial_tile_lanes_are_masked exists.
A second round of mutants, for the hand-written tables of icp_cases (rule_cases, solve_cases, batch300); none of them is
seen by any case above:
  * roundf for rintf: fails the four `ties` frames of the rule table;
  * (n.n) < 1.5f, the test dropped, or written as `> 1.5f rejects` (a NaN passes): fail even.model;
  * e.e < dist2 fails even.dist; written as `> dist2 rejects` it fails even.model (e.e is NaN under a model depth of +Inf
    on the row of cy); q.q < reach2 fails even.reach; Mz >= 0 fails even.model;
  * `s >= thr` in icp_cholesky fails pivot0_equal and pivot5_zero; `count <= min_corr` fails min_corr_equal;
  * k_icp_prepare stopping at lane 256 fails batch300.
  Not seen by anything, because a later test of rule 3 rejects what these let through: the depth range, q_z > 0 or the
  reach test letting a NaN pass, q_z >= 0, um > -1 for um >= 0, and the zero normal written as N == 0 on all three."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC   # noqa: E402
from aria_slam_amd import icp_ref as IR   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


def emu_source():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "icp_track.hip")).read()
    body = src[src.index("\nnamespace {"):src.index("\n}  // namespace\n\n// ---- C-ABI")]
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("icp_kernel_emu_head.inc", "icp_kernel_emu_tail.inc")]
    return parts[0], body, parts[1]


def build_emu(body=None, tag="icp_emu"):
    head, text, tail = emu_source()
    out_dir = os.path.join(ROOT, "build", tag)
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, tag + ".cpp"), os.path.join(out_dir, "lib%s.so" % tag)
    with open(cpp, "w") as f:
        f.write(head + (body or text) + tail)
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-o", so, cpp])
    L = C.CDLL(so)
    p, i = C.c_void_p, C.c_int
    L.emu_icp_system.argtypes = [p, p, p, i, p, p, p, p, i, i, i, i, i, p]
    L.emu_icp_system.restype = None
    L.emu_icp_track.argtypes = [p, p, p, i, i, p, p, p, p, p, p, p, i, i, i, i, p, p, p]
    L.emu_icp_track.restype = None
    return L


@pytest.fixture(scope="module")
def emu():
    body = emu_source()[1]
    for k in ("k_icp_prepare", "k_icp_accumulate", "k_icp_solve", "k_icp_export", "icp_pixel", "icp_cholesky"):
        assert k in body, k
    assert "asm" not in body and "__shared__" not in body and "__syncthreads" not in body, "plain HIP C++, no LDS, no barrier"
    assert "__shfl" not in body and "atomicAdd" not in body, "the cross-lane commit stays outside the pasted text"
    return build_emu()


def _args(cfg, b, lay, live_fill=None):
    """The argument blocks of the drivers; the first element keeps every array alive."""
    inp = IC.pack(b, lay, live_fill)
    K = np.array(cfg.K, np.float64)
    fp = np.array([cfg.min_depth, cfg.max_depth, cfg.dist_max, cfg.reach], np.float32)
    dp = np.array([cfg.min_pivot, cfg.eps], np.float64)
    maps = (C.c_void_p * 3)(inp["live"].ctypes.data, inp["depth"].ctypes.data, inp["normal"].ctypes.data)
    l = np.array([lay["live"][1], lay["depth"][1], lay["normal"][1], lay["live"][0], lay["depth"][0], lay["normal"][0]], np.int64)
    return (inp, K, fp, dp, maps, l), (K.ctypes.data, fp.ctypes.data, dp.ctypes.data, cfg.min_corr), (C.addressof(maps), l.ctypes.data)


def system(L, cfg, b, lay, trel, stride, plain=0, live_fill=None):
    keep, head, maps = _args(cfg, b, lay, live_fill)
    n = len(b.frames)
    trel = np.ascontiguousarray(trel, np.float64)
    out = np.zeros((n, IR.N_TERMS), np.int64)
    L.emu_icp_system(*head, *maps, keep[0]["Tm"].ctypes.data, trel.ctypes.data, n, b.W, b.H, stride, plain, out.ctypes.data)
    return out, keep[0]


def track(L, cfg, b, lay, plain=0):
    keep, head, maps = _args(cfg, b, lay)
    n = len(b.frames)
    poses, recs = IC.guarded_outputs(n)
    err = np.zeros(1, np.int32)
    strides, its = np.array(cfg.strides, np.int32), np.array(cfg.iterations, np.int32)
    L.emu_icp_track(*head, len(cfg.strides), strides.ctypes.data, its.ctypes.data, *maps, keep[0]["Tm"].ctypes.data,
                    keep[0]["T0"].ctypes.data, None if b.mask is None else b.mask.ctypes.data, n, b.W, b.H, plain, poses.ctypes.data,
                    recs.ctypes.data, err.ctypes.data)
    return poses, recs, int(err[0]), keep[0]


@pytest.mark.parametrize("plain", (0, 1))
@pytest.mark.parametrize("name", IC.SINGLES)
def test_system_kernel_source_is_the_restatements_integers_at_every_level(emu, name, plain):
    f = IC.frame(name)
    cfg = IC.config(f.K)
    b = IC.batch([name])
    lay = IC.layout(f.W, f.H, padded=name == "pitched")
    trel = IR.relative(f.Tm, f.T0)
    for stride in (4, 2, 1, 16):
        got, inp = system(emu, cfg, b, lay, [trel], stride, plain)
        want = IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)
        assert (got[0] == want).all(), (stride, got[0] - want)
        assert want[28] > 0 or name == "tiny"
    for key in ("live", "depth", "normal"):
        assert inp[key].tobytes() == IC.pack(b, lay)[key].tobytes()


@pytest.mark.parametrize("plain", (0, 1))
def test_partial_tile_lanes_are_masked(emu, plain):
    """`edge`: valid depths in the live map's padding, which only a lane outside W x H can read."""
    cfg, b, lay, trel = IC.edge_case()
    f = b.frames[0]
    for stride in (4, 2, 1):
        got, _ = system(emu, cfg, b, lay, [trel], stride, plain, live_fill=IC.EDGE_DEPTH)
        want = IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)
        assert (got[0] == want).all() and want[28] > 0, (stride, got[0][28], want[28])
    assert want[28] == (IC.WO - 2) * (IC.HO - 2)


@pytest.mark.parametrize("plain", (0, 1))
@pytest.mark.parametrize("name", IC.SINGLES)
def test_track_kernel_source_is_bitwise_the_restatement(emu, name, plain):
    f = IC.frame(name)
    cfg = IC.config(f.K)
    b = IC.batch([name])
    lay = IC.layout(f.W, f.H, padded=name == "pitched")
    poses, recs, err, _ = track(emu, cfg, b, lay, plain)
    want = IC.expected(b, cfg)
    assert recs.tobytes() == want[1].tobytes(), (recs, want[1])
    assert poses.tobytes() == want[0].tobytes()
    assert err == 0 and int(recs[0]["valid"]) == (0 if name in IC.LOST else 1)


@pytest.mark.parametrize("levels", IC.LEVELS)
def test_track_kernel_source_levels(emu, levels):
    b = IC.batch(["corner"])
    cfg = IC.config(IC.K, **levels)
    poses, recs, err, _ = track(emu, cfg, b, IC.layout(b.W, b.H))
    want = IC.expected(b, cfg)
    assert recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes() and err == 0
    assert int(recs[0]["iterations_run"]) >= 1


def test_track_kernel_source_batch_of_five_masked_and_nonfinite(emu):
    """The five frames of one shape in one batch, at every position; two of them masked (their bytes keep the guard); a NaN in
    T0 of one frame (a zero record, no pose, the error bit; the others unaffected)."""
    cfg = IC.config(IC.K)
    lay = IC.layout(IC.W, IC.H)
    for shift in range(5):
        names = IC.FIVE[shift:] + IC.FIVE[:shift]
        b = IC.batch(names)
        poses, recs, err, _ = track(emu, cfg, b, lay)
        want = IC.expected(b, cfg)
        assert err == 0 and recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes(), shift
    b = IC.batch(IC.FIVE, mask=[1, 0, 1, 1, 0])
    poses, recs, err, _ = track(emu, cfg, b, lay)
    want = IC.expected(b, cfg)
    assert err == 0 and recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
    guard_p, guard_r = IC.guarded_outputs(5)
    for f in (1, 4):
        assert poses[f].tobytes() == guard_p[f].tobytes() and recs[f:f + 1].tobytes() == guard_r[f:f + 1].tobytes()
    b = IC.batch(["corner", "corner", "converged"], nan_frame=1)
    poses, recs, err, _ = track(emu, cfg, b, IC.layout(b.W, b.H))
    want = IC.expected(b, cfg)
    assert err == 1 and want[2]
    assert recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
    assert recs[1:2].tobytes() == bytes(32) and poses[1].tobytes() == IC.guarded_outputs(1)[0].tobytes()


@pytest.mark.parametrize("plain", (0, 1))
@pytest.mark.parametrize("group", (0, 1), ids=("even", "odd"))
def test_rule_table_kernel_source_is_the_restatements_integers(emu, group, plain):
    """The hand-written pixels of icp_cases.rule_cases(): every frame of a group in one call, each at its own Trel, dense and
    with valid depths in the live map's padding, at strides 1 and 2."""
    g = IC.rule_cases()[group]
    for padded in (False, True):
        lay = IC.layout(g.batch.W, g.batch.H, padded)
        for stride in (1, 2):
            got, _ = system(emu, g.cfg, g.batch, lay, g.trels, stride, plain, live_fill=1.0 if padded else None)
            want = IC.rule_systems(g, stride)
            bad = [g.batch.frames[i].name for i in range(len(want)) if (got[i] != want[i]).any()]
            assert not bad, (padded, stride, bad)


@pytest.mark.parametrize("plain", (0, 1))
def test_solve_table_kernel_source_is_bitwise_the_restatement(emu, plain):
    for c in IC.solve_cases():
        b = IC.Batch([c.frame], None, c.frame.W, c.frame.H, c.frame.K)
        poses, recs, err, _ = track(emu, c.cfg, b, IC.layout(b.W, b.H), plain)
        want = IC.solve_ref(c)[0]
        assert err == 0 and recs[0].tobytes() == want.result.tobytes(), (c.name, recs[0], want.result)
        assert poses[0].tobytes() == want.T.tobytes(), c.name


def test_batch_of_300_kernel_source_second_block_of_the_per_frame_kernels(emu):
    """Frames 256 .. 299 belong to the second block of k_icp_prepare and k_icp_solve; masked, lost and non-finite frames on both
    sides of it."""
    cfg, b = IC.batch300()
    poses, recs, err, _ = track(emu, cfg, b, IC.layout(b.W, b.H))
    want = IC.expected(b, cfg)
    assert err == 1 and want[2]
    assert recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()


def test_bound_case_kernel_source_is_the_restatements_integers(emu):
    cfg, D, M, N, trel, Rm = IC.bound_case()
    f = IC.Frame("bound", D, M, N, IC.IDENTITY, IC.IDENTITY, IC.IDENTITY, 4, 4, cfg.K)
    got, _ = system(emu, cfg, IC.Batch([f], None, 4, 4, cfg.K), IC.layout(4, 4), [trel], 1)
    want = IR.system(cfg, D, M, N, trel, Rm, 1)
    assert (got[0] == want).all() and np.abs(want[:21]).max() > 2.0 ** 37
