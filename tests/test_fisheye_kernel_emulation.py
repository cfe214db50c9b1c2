"""The fisheye (KB4) kernels of aria_slam_amd/csrc/rectify.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/rectify_ref.py) on the cases of fisheye_cases.py that tests/test_gpu_fisheye.py runs on the device.

The recipe is test_rectify_kernel_emulation.py's: the text of the file between "namespace {" and the C-ABI is pasted between
tests/cpp/rect_kernel_emu_head.inc and the tails rect_kernel_emu_tail.inc + rect_kb4_emu_tail.inc and compiled with the
clang++ that hipcc drives, at -O1 -ffp-contract=off. Without a GPU this checks the indexing, the order of the fp64
operations of rect_atan, rect_tan, P and D as the host compiler takes them, the validity rules, and -- the fisheye maps
going through the shim's k_rect_remap in the same build -- that no load leaves the source images on maps of this model.
It also pins the text of the three radtan / remap kernels to the commit before the fisheye model: they are not edited."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisheye_cases as F   # noqa: E402
import rectify_cases as RC   # noqa: E402
from aria_slam_amd import rectify_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
# SHA-256 of each kernel's text, from the line of its __global__ to its closing brace, at the commit before the fisheye model
PARENT_SHA256 = {
    "k_rect_build_map": "f3ef62764dfb4f2ecd558540ab2f4a96d22fe253d5a2e762572602735c435192",
    "k_rect_points": "4662c15aa187a82f4a00387e642a6983bd1777146064df094aa0f34761342f37",
    "k_rect_remap": "3ef5a4426d0126c0e025c8f75191081c571987c565e2ba37a405d0395a2b56c3",
}


def _source():
    return open(os.path.join(ROOT, "aria_slam_amd", "csrc", "rectify.hip")).read()


def _kernel_text(src, name):
    i = src.index("void %s(" % name)
    return src[src.rindex("\n", 0, i) + 1:src.index("\n}\n", i) + 3]


def test_radtan_and_remap_kernels_are_not_edited():
    src = _source()
    for name, want in PARENT_SHA256.items():
        text = _kernel_text(src, name)
        assert text.startswith("__global__") and text.endswith("\n}\n")
        assert hashlib.sha256(text.encode()).hexdigest() == want, name


@pytest.fixture(scope="module")
def emu():
    src = _source()
    body = src[src.index("\nnamespace {"):src.index("\n// ---- C-ABI")]
    for name in ("k_rect_build_map_kb4", "k_rect_points_kb4", "rect_atan", "rect_tan", "rect_kb4_P", "rect_kb4_D"):
        assert name in body, "%s is not in the anonymous namespace before the C-ABI" % name
    assert "asm" not in body and "__shared__" not in body.split("#ifdef ARIA_VARIANTS")[0], "plain HIP C++, no LDS"
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read()
             for n in ("rect_kernel_emu_head.inc", "rect_kernel_emu_tail.inc", "rect_kb4_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "rect_kb4_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "rect_kb4_emu.cpp"), os.path.join(out_dir, "librect_kb4_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + parts[1] + parts[2])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, cpp])
    L = C.CDLL(so)
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.emu_build_map_kb4.argtypes = [p, i, i, i, i, p]
    L.emu_remap.argtypes = [p, i, i, p, i64, i, i, i, i, i, i, p, i64, i, i]
    L.emu_points_kb4.argtypes = [p, p, p, i64, i, p, p]
    L.emu_bad_loads.restype = C.c_long
    return L


def _cam_args(cam, new_K):
    return np.array(list(cam["K"]) + list(cam["dist"]) + list(cam["R"]) + list(new_K), np.float64)


def _emu_map(L, case):
    pitch = L.emu_map_pitch(case.dst[0])
    raw = np.zeros(pitch * case.dst[1] * 4 + 64, np.uint8)
    off = (-raw.ctypes.data) % 16                                  # 16-byte aligned, as a device allocation is
    m = raw[off:off + 4 * pitch * case.dst[1]].view(np.uint32)
    m[:] = 0x12345678
    a = _cam_args(case.cam, case.new_K)
    L.emu_build_map_kb4(a.ctypes.data, case.src[0], case.src[1], case.dst[0], case.dst[1], m.ctypes.data)
    return m, pitch


@pytest.fixture(scope="module")
def case_maps(emu):
    return {name: _emu_map(emu, case) for name, case in F.CASES.items()}


@pytest.mark.parametrize("name", list(F.CASES))
def test_map_kernel_source_is_bitwise_the_restatement(case_maps, name):
    """Every case of fisheye_cases.CASES; the padded columns of a map row are invalid."""
    case = F.CASES[name]
    m, pitch = case_maps[name]
    m = m.reshape(case.dst[1], pitch)
    assert m[:, :case.dst[0]].tobytes() == case.map.tobytes(), (name, int((m[:, :case.dst[0]] != case.map).sum()))
    assert (m[:, case.dst[0]:] == R.INVALID).all()
    assert pitch > case.dst[0] or case.dst[0] % 4 == 0


def test_zoom10_reaches_both_loaded_read_forms():
    """Of zoom10's 720 lanes 147 have no valid pixel, 255 take the ROWS form and 318 the TAPS form (fold8: 135 / 277 / 308)."""
    form = F.read_forms(F.CASES["zoom10"].map, F.SRC[0])["form"]
    assert ((form == RC.NONE).sum(), (form == RC.ROWS).sum(), (form == RC.TAPS).sum()) == (147, 255, 318)


def _case_remap(L, case, m, frames, group, rows_ok=1):
    n = len(frames)
    src = case.src_buffer(frames)
    dst = np.full(n * case.dst_stride, 0x5A, np.uint8)
    L.emu_remap(m.ctypes.data, case.dst[0], case.dst[1], src.ctypes.data, case.src_stride, case.src_pitch, case.src[0], case.src[1],
                rows_ok, n, group, dst.ctypes.data, case.dst_stride, case.dst_pitch, case.fill)
    bad = L.emu_bad_loads()
    assert bad == 0, "%s: %d loads left the source images" % (case.name, bad)
    img, pad_kept = case.images(dst, n)
    assert pad_kept, "padding was written"
    return img


@pytest.mark.parametrize("name", list(F.CASES))
def test_remap_of_fisheye_maps_is_bitwise_the_restatement(emu, case_maps, name):
    """Nine noise frames (groups of 8 and 1) through the unchanged k_rect_remap on the emulated fisheye map: the shipped
    group, the tap loads forced, a group of 3; the lone frame of the second group in a call of its own."""
    case = F.CASES[name]
    m = case_maps[name][0]
    assert case.n_frames == 9 and emu.emu_group() == 8
    for group, rows_ok in ((emu.emu_group(), 1), (emu.emu_group(), 0), (3, 1)):
        got = _case_remap(emu, case, m, case.frames, group, rows_ok)
        assert got.tobytes() == case.want.tobytes(), (name, group, rows_ok, int((got != case.want).sum()))
    assert _case_remap(emu, case, m, case.frames[8:9], emu.emu_group()).tobytes() == case.want[8:9].tobytes()


@pytest.mark.parametrize("name,cam", F.point_cameras(), ids=[n for n, _ in F.point_cameras()])
def test_points_kernel_source_is_bitwise_the_restatement(emu, name, cam):
    """Records around and far outside the image with the non-finite head: (-1, -1) exactly where the restatement says; in
    place equals out of place; records beyond the count untouched; a bad count skips its frame and raises the error bit."""
    kp, counts = F.keypoints(), F.POINT_COUNTS
    want = F.ref_points_all()[name]
    a = _cam_args(cam, cam["K"])
    out = np.frombuffer(bytes([0x5A]) * kp.nbytes, np.uint8).copy().view(kp.dtype).reshape(kp.shape)
    err = np.zeros(1, np.int32)
    emu.emu_points_kb4(a.ctypes.data, kp.ctypes.data, counts.ctypes.data, F.KP_STRIDE, 2, out.ctypes.data, err.ctypes.data)
    assert err[0] == 0
    for f, n in enumerate(counts):
        assert out[f, :n].tobytes() == want[f, :n].tobytes(), (name, f, int((out[f, :n] != want[f, :n]).sum()))
        assert (out[f, n:].view(np.uint8) == 0x5A).all()
    inplace = kp.copy()
    emu.emu_points_kb4(a.ctypes.data, inplace.ctypes.data, counts.ctypes.data, F.KP_STRIDE, 2, inplace.ctypes.data, err.ctypes.data)
    assert inplace.tobytes() == want.tobytes() and err[0] == 0
    for bad in (np.array([-1, F.KP_STRIDE], np.int32), np.array([F.KP_STRIDE + 1, 1], np.int32)):
        inplace, err[0] = kp.copy(), 0
        emu.emu_points_kb4(a.ctypes.data, inplace.ctypes.data, bad.ctypes.data, F.KP_STRIDE, 2, inplace.ctypes.data, err.ctypes.data)
        assert err[0] == 1 and inplace[0].tobytes() == kp[0].tobytes()
        assert inplace.tobytes() == F.ref_points(cam, kp, bad).tobytes()
