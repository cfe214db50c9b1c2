"""The kernel source of aria_slam_amd/csrc/proj_search.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/proj_ref.py) on the case table tests/test_gpu_proj.py runs on the device, and on every limit and size of
edge_groups() (tests/test_gpu_proj_edges.py) under each group's own configuration.

Three pieces of the file's text are pasted between tests/cpp/proj_kernel_emu_head.inc (a shim: the lanes of a workgroup one after
the other) and proj_kernel_emu_tail.inc and compiled with the clang++ that hipcc drives: the plain per-landmark arithmetic between
the file's two marker comments (projection, candidate test, descriptor distance, running top-2 and its merge, acceptance, the
cell of a coordinate, the claim key), k_proj_resolve and k_proj_from_map. The tail restates the search around those functions,
offers the keypoints in both orders and in two merged halves (the top-2 may depend on no order), and counts candidates outside
the cell range the kernel walks (none: the binning cannot lose one).

What this cannot check is what has LDS, barriers or cross-lane operations -- the counting sort of k_proj_bin, the 16-lane walk
and the shuffles of k_proj_search, the ballot compaction of k_proj_compact -- and the device's streams and lifecycle: that is
tests/test_gpu_proj.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_cases as PC   # noqa: E402
from aria_slam_amd import proj_ref as R   # noqa: E402
from aria_slam_amd._lib import KP_DTYPE, MAP_POINT_DTYPE, PROJ_LANDMARK_DTYPE, PROJ_OBS_DTYPE   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


def _kernel_text(src, name):
    """The text of a __global__ kernel from its template-free header to the closing brace in column 0."""
    start = src.index("__global__ __launch_bounds__(PJ_BLOCK) void %s(" % name)
    return src[start:src.index("\n}\n", start) + 3]


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "proj_search.hip")).read()
    plain = src[src.index("// ---- the plain per-landmark arithmetic"):src.index("// ---- end of the plain arithmetic ----")]
    for fn in ("proj_project", "proj_candidate", "proj_hamming", "proj_top2", "proj_top2_merge", "proj_decide", "proj_cell", "proj_claim_key"):
        assert fn in plain, fn
    body = plain + _kernel_text(src, "k_proj_resolve") + _kernel_text(src, "k_proj_from_map")
    for word in ("__shared__", "__syncthreads", "__shfl", "__ballot", "asm"):
        assert word not in body, "plain HIP C++: no LDS, no barrier, no cross-lane operation (%s)" % word
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("proj_kernel_emu_head.inc", "proj_kernel_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "proj_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "proj_emu.cpp"), os.path.join(out_dir, "libproj_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + parts[1])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I", os.path.join(ROOT, "include"),
                           "-o", so, cpp])
    L = C.CDLL(so)
    p, i, i64, d, f = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_float
    L.emu_search.argtypes = [p, p, p, i, i64, i, i, p, i, i, i, p, d, f, f, i, i, p, p, p]
    L.emu_from_map.argtypes = [p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, i, i, p, p, p, i64, i, p, p, p]
    L.emu_from_map.restype = None
    L.emu_is_finite.argtypes = [d]
    return L


def _search(L, pose, kp, desc, n, kp_stride, width, height, landmarks, first, count, land_cap, cfg):
    c = dict(R.DEFAULTS, **cfg)
    pose = np.ascontiguousarray(pose, np.float64)
    kp, desc = np.ascontiguousarray(kp), np.ascontiguousarray(desc, np.uint8)
    lm = np.ascontiguousarray(landmarks)
    K, scale = np.array(c["K"], np.float64), R.level_scales()
    obs = np.zeros(land_cap + 1, PROJ_OBS_DTYPE)
    obs.view(np.uint8)[:] = 0x5A
    claims = np.full(max(kp_stride, 1), -7, np.int32)
    outside = L.emu_search(pose.ctypes.data, kp.ctypes.data, desc.ctypes.data, n, kp_stride, width, height, lm.ctypes.data, first, count,
                           land_cap, K.ctypes.data, c["min_depth"], c["radius_px"], c["ratio"], c["th_hamming"], c["max_octave_diff"],
                           scale.ctypes.data, obs.ctypes.data, claims.ctypes.data)
    assert (obs[land_cap:].view(np.uint8) == 0x5A).all(), "a record beyond land_cap was touched"
    return obs[:land_cap], outside


def _valid_frames():
    return [pytest.param(f, id=f["name"]) for f in PC.table()["frames"] if f["valid"]]


@pytest.mark.parametrize("f", _valid_frames())
def test_plain_arithmetic_and_resolve_are_bitwise_the_restatement(emu, f):
    t = PC.table()
    kp, desc = PC.frame_arrays(f)
    got, outside = _search(emu, f["pose"], kp, desc, f["n"], t["kp_stride"], t["width"], t["height"], t["landmarks"], f["first"], f["count"],
                           t["land_cap"], t["cfg"])
    want = R.search_frame_ref(f["pose"], kp, desc, f["n"], t["kp_stride"], t["landmarks"], f["first"], f["count"], t["land_cap"], t["cfg"],
                              t["width"], t["height"])[0]
    assert outside == 0
    assert got.tobytes() == want.tobytes() == PC.expected(f, t["landmarks"])[0].tobytes(), f["name"]


def _edge_frames():
    return [pytest.param(g, f, id="%s / %s" % (g["name"], f["name"])) for g in PC.edge_groups() for f in g["frames"] if f["valid"]]


@pytest.mark.parametrize("g,f", _edge_frames())
def test_plain_arithmetic_on_every_limit_and_size(emu, g, f):
    """Every valid frame of edge_groups() under its group's configuration, image size, kp_stride and land_cap. claim_bits passes
    its whole range of 2^20 landmarks (the dead ones return at the first test, so the range costs a fraction of a second).
    outside == 0 is the check that one pixel of slack around the window suffices: for the differences of the fp32 group that
    round ONTO r, and for the radius_px = 1024 windows, whose edges lie a thousand pixels outside the image."""
    kp, desc = PC.edge_frame_arrays(g, f)
    got, outside = _search(emu, f["pose"], kp, desc, f["n"], g["kp_stride"], g["width"], g["height"], g["landmarks"], f["first"], f["count"],
                           g["land_cap"], g["cfg"])
    assert outside == 0
    assert got.tobytes() == PC.edge_restatement(g, f)[0].tobytes() == PC.edge_expected(g, f)[0].tobytes(), (g["name"], f["name"])


def test_crowded_random_scene_in_large_coordinates(emu):
    """1408 x 1408, every octave, keypoints a little outside the image, NaN coordinates: ties, rejections and lost claims."""
    rng = np.random.default_rng(8)
    NK, NL, S = 700, 900, 1408
    pool = R.random_descriptors(rng, 12)
    kp = np.zeros(NK, KP_DTYPE)
    kp["x"], kp["y"] = rng.uniform(-40, S + 40, NK).astype(np.float32), rng.uniform(-40, S + 40, NK).astype(np.float32)
    kp["x"][:3], kp["y"][3:6] = np.nan, np.inf
    kp["octave"] = rng.integers(-1, 10, NK)
    desc = pool[rng.integers(0, 12, NK)].copy()
    desc[:, 0] ^= rng.integers(0, 256, NK).astype(np.uint8) * (rng.random(NK) < 0.6)
    K = (700.0, 700.0, 704.0, 704.0)
    lm = np.zeros(NL, PROJ_LANDMARK_DTYPE)
    z = rng.uniform(0.05, 9.0, NL)
    u, v = rng.uniform(-30, S + 30, NL), rng.uniform(-30, S + 30, NL)
    lm["X"] = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    lm["desc"], lm["octave"] = pool[rng.integers(0, 12, NL)], rng.integers(-1, 9, NL)
    pose = np.array([1, 0, 0, 0.01, 0, 1, 0, 0.02, 0, 0, 1, 0.05], np.float64)
    cfg = dict(K=K, radius_px=40.0)
    got, outside = _search(emu, pose, kp, desc, NK, NK, S, S, lm, 0, NL, NL, cfg)
    want = R.search_frame_ref(pose, kp, desc, NK, NK, lm, 0, NL, NL, cfg, S, S)[0]
    assert outside == 0 and got.tobytes() == want.tobytes()
    assert {0, 1, 3, 7, 15} <= set(want["flags"].tolist())


def test_from_map_kernel_is_the_restatement(emu):
    rng = np.random.default_rng(3)
    n_slots, stride, size = 4, 40, 700
    kp = np.zeros((n_slots, stride), KP_DTYPE)
    kp["octave"] = rng.integers(0, 8, (n_slots, stride))
    desc = R.random_descriptors(rng, n_slots * stride).reshape(n_slots, stride, 32)
    n = np.array([40, 25, 0, 41], np.int32)                                   # slot 3 claims more than the stride: every point of it is refused
    arena = np.zeros(size + 50, MAP_POINT_DTYPE)
    arena["pair"] = rng.integers(8, 15, len(arena))                           # slots -2 .. 4 under pair_base 10
    arena["idx1"], arena["idx2"] = rng.integers(-2, 45, len(arena)), rng.integers(-2, 45, len(arena))
    arena["X"] = rng.normal(size=(len(arena), 3))
    for first, max_count, view, slots in ((0, size, 2, n_slots), (100, 300, 1, n_slots), (650, 100, 2, 2), (size + 3, 9, 1, n_slots), (0, 0, 2, n_slots)):
        want, cnt, invalid = R.landmarks_from_map_ref(arena, size, first, max_count, 10, view, kp, desc, n, stride, slots)
        got = np.zeros(max_count + 1, PROJ_LANDMARK_DTYPE)
        got.view(np.uint8)[:] = 0x5A
        nland, err = np.full(1, -7, np.int32), np.zeros(1, np.int32)
        emu.emu_from_map(arena.ctypes.data, size, len(arena), first, max_count, 10, view, kp.ctypes.data, desc.ctypes.data, n.ctypes.data,
                         stride, slots, got.ctypes.data, nland.ctypes.data, err.ctypes.data)
        assert nland[0] == cnt and got[:max_count].tobytes() == want.tobytes(), (first, max_count, view)
        assert (got[max_count:].view(np.uint8) == 0x5A).all() and err[0] == (1 if invalid else 0)


def test_pose_entries_that_are_not_finite(emu):
    for v, want in ((0.0, 1), (-1e308, 1), (5e-324, 1), (float("inf"), 0), (float("-inf"), 0), (float("nan"), 0)):
        assert emu.emu_is_finite(v) == want, v
