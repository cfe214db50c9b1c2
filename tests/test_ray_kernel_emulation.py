"""The kernel source of aria_slam_amd/csrc/tsdf_raycast.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/ray_ref.py) on the shapes (a), (b) and (c) tests/test_gpu_ray.py runs on the device, with skip = 1 and 0.

The text of the file between "namespace {" and the C-ABI section -- k_ray_prepare, k_ray_bricks, k_ray_brick_words, k_ray_march, k_ray_finish
and their device functions -- is pasted between tests/cpp/ray_kernel_emu_head.inc (a shim: the lanes of a workgroup one after the
other; the kernels have no barrier; the view record's cross-lane tally served lane by lane) and ray_kernel_emu_tail.inc (the
parameters and the launch geometry) and compiled with the clang++ that hipcc drives. What this checks without a GPU is the
indexing, the tile geometry, the order of the fp32 operations as the host compiler takes them, the padded layouts, the brick
bits and, above all, that the clip bounds drop no sample the restatement (which does not clip) sees; what it cannot check is
the device's arithmetic, the wave tally and the streams: that is tests/test_gpu_ray.py.

Mutants, each put into the pasted text by hand and run once against this file (not committed):
  * the clip margin set to zero (m = 0 in ray_clip, with or without kmargin = 0 in ray_params): fails `grazing`, whose first
    ray runs along the face x = -0.5 of the box tilted outward by less than an ulp: its computed g_x stays exactly -0.5, which
    rintf takes inside, while the unwidened slab ends at z = -0 and leaves no sample. The widened slabs are the only thing
    that keeps such rays; no fused scene has one. kmargin = 0 alone changes no byte of any case: the slab margin, mapped to
    z, exceeds the rounding of z_k by four orders of magnitude, so the sample margin is a second guard, not the first;
  * the range cut short (kmargin = -2), or the box one voxel short at its low or its high faces: fail scene, small, many,
    yaw_pitch, the three range cases with hits and slab;
  * sample k - 1 not re-fetched (recA taken as a zero record): every case with a hit fails;
  * the brick flag taken from tsdf <= 0 instead of tsdf < 0: no plane changes, and none can: it sets a superset of the bits,
    which costs loads and changes no byte; the words themselves differ on slab (its minus zero), which
    test_brick_words_are_the_bricks_with_a_seen_negative_voxel sees. Its dual, the flag taken from tsdf < -0.25 (a subset),
    fails slab; the brick index with x and y swapped fails scene, narrow, yaw_pitch and the range cases."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_cases as RC   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
CASES = RC.all_cases()


def emu_source():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "tsdf_raycast.hip")).read()
    body = src[src.index("\nnamespace {"):src.index("\n}  // namespace\n\n// ---- C-ABI")]
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("ray_kernel_emu_head.inc", "ray_kernel_emu_tail.inc")]
    return parts[0], body, parts[1]


def build_emu(body=None, tag="ray_emu"):
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
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.emu_ray_steps.argtypes = [p, p, p]
    L.emu_ray_words.argtypes = [p]
    L.emu_ray_bricks.argtypes = [p, p, p, p, p]
    L.emu_ray_bricks.restype = None
    L.emu_ray_cast.argtypes = [p, p, p, p, p, p, p, i, i, i, p, i64, i, p, i64, i, p, i64, i, p, i64, i, p, p]
    L.emu_ray_cast.restype = None
    return L


@pytest.fixture(scope="module")
def emu():
    body = emu_source()[1]
    for k in ("k_ray_prepare", "k_ray_bricks", "k_ray_brick_words", "k_ray_march", "k_ray_finish", "ray_clip"):
        assert k in body, k
    assert "asm" not in body and "__shared__" not in body and "__syncthreads" not in body, "plain HIP C++, no LDS, no barrier"
    assert "__shfl" not in body and "__ballot" not in body, "the cross-lane tally stays outside the pasted text"
    return build_emu()


def _params(cfg, skip):
    ip = np.array(list(cfg.dims) + [cfg.min_weight, skip], np.int32)
    fp = np.array([cfg.voxel, *cfg.origin, cfg.near, cfg.far, cfg.step], np.float32)
    return ip, fp, np.array(cfg.K, np.float64)


def run(L, case, layout, planes=RC.PLANES, skip=1, views=True):
    """One update and one cast of the emulated kernels into guarded buffers: ({plane: buffer, "views": records}, error word)."""
    ip, fp, K = _params(case.cfg, skip)
    vol = np.ascontiguousarray(case.vol)
    words = np.zeros(L.emu_ray_words(ip.ctypes.data), np.uint32)
    L.emu_ray_bricks(ip.ctypes.data, fp.ctypes.data, K.ctypes.data, vol.ctypes.data, words.ctypes.data)
    out = RC.guarded(case, layout, planes)
    err = np.zeros(1, np.int32)
    ext = np.ascontiguousarray(case.ext, np.float64)
    args = []
    for p in RC.PLANES:
        args += [out[p].ctypes.data if p in planes else None, layout[p][1], layout[p][0]]
    L.emu_ray_cast(ip.ctypes.data, fp.ctypes.data, K.ctypes.data, vol.ctypes.data, words.ctypes.data, ext.ctypes.data,
                   case.mask.ctypes.data if case.mask is not None else None, len(ext), case.W, case.H, *args,
                   out["views"].ctypes.data if views else None, err.ctypes.data)
    return out, int(err[0])


def test_emulated_n_steps_equal_the_restatement(emu):
    for case in CASES.values():
        ip, fp, K = _params(case.cfg, 1)
        assert emu.emu_ray_steps(ip.ctypes.data, fp.ctypes.data, K.ctypes.data) == RC.RR.n_steps(case.cfg), case.name


@pytest.mark.parametrize("skip", (1, 0))
@pytest.mark.parametrize("name", sorted(CASES))
def test_march_kernel_source_is_bitwise_the_restatement(emu, name, skip):
    """Shapes (a), (b), (c): every plane and every view record, dense."""
    case = CASES[name]
    layout = RC.dense_layout(case.W, case.H)
    got, err = run(emu, case, layout, skip=skip)
    assert RC.same_bytes(got, RC.expected(case, layout)) == {}
    assert err == (1 if RC.ref(case)[1] else 0)


def test_march_kernel_source_scene_bad_and_masked_views(emu):
    """Shape (a): the masked view keeps the guard, the view with an Inf extrinsic is zero with valid = 0 and raises the error
    bit; each good view alone gives the bytes it has in the batch."""
    case = RC.scene()
    layout = RC.dense_layout(case.W, case.H)
    got, err = run(emu, case, layout)
    assert err == 1 and RC.ref(case)[1]
    assert (np.frombuffer(got["depth"][4].tobytes(), np.uint8) == RC.GUARD).all()
    assert (np.frombuffer(got["views"][4:5].tobytes(), np.uint8) == RC.GUARD).all()
    assert not got["depth"][5].any() and not got["normal"][5].any() and not got["gray"][5].any() and not got["shade"][5].any()
    assert got["views"][5].tobytes() == bytes(16)
    for i in range(4):
        one, err = run(emu, RC.scene_single(i), layout)
        assert err == 0
        for k in RC.PLANES + ("views",):
            assert one[k][0].tobytes() == got[k][i].tobytes(), (i, k)


@pytest.mark.parametrize("name", ("small_view", "many_tiny"))
def test_march_kernel_source_padded_layouts_and_null_planes(emu, name):
    """Shape (b): padded pitches and strides on every plane with a guard that survives; every combination of one NULL plane;
    no view records."""
    case = CASES[name]
    layout = RC.padded_layout(case.W, case.H)
    for skip in (1, 0):
        got, _ = run(emu, case, layout, skip=skip)
        assert RC.same_bytes(got, RC.expected(case, layout)) == {}
    for drop in RC.PLANES:
        planes = tuple(p for p in RC.PLANES if p != drop)
        got, _ = run(emu, case, layout, planes)
        assert RC.same_bytes(got, RC.expected(case, layout, planes)) == {}, drop
    got, _ = run(emu, case, layout, views=False)
    want = RC.expected(case, layout)
    want["views"] = RC.guarded(case, layout)["views"]
    assert RC.same_bytes(got, want) == {}


def test_brick_words_are_the_bricks_with_a_seen_negative_voxel(emu):
    for name in ("scene", "small_view", "slab", "grazing"):
        case = CASES[name]
        ip, fp, K = _params(case.cfg, 1)
        vol = np.ascontiguousarray(case.vol)
        words = np.zeros(emu.emu_ray_words(ip.ctypes.data), np.uint32)
        emu.emu_ray_bricks(ip.ctypes.data, fp.ctypes.data, K.ctypes.data, vol.ctypes.data, words.ctypes.data)
        nx, ny, nz = case.cfg.dims
        flag = (vol["weight"] >= case.cfg.min_weight) & (vol["tsdf"] < 0)
        bricks = flag.reshape(nz // 8, 8, ny // 8, 8, nx // 8, 8).any(axis=(1, 3, 5)).reshape(-1)
        bits = (words[np.arange(bricks.size) >> 5] >> (np.arange(bricks.size) & 31).astype(np.uint32)) & 1
        assert (bits.astype(bool) == bricks).all()
        assert 0 < bricks.sum() and (name != "scene" or bricks.sum() < bricks.size)
