"""The kernel source of aria_slam_amd/csrc/rectify.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/rectify_ref.py) on the shapes (a)-(d) and the read-form and edge cases (rectify_cases.EDGE_CASES)
tests/test_gpu_rectify.py runs on the device.

The text of the file between "namespace {" and the C-ABI -- the three kernels and their device functions -- is pasted
between tests/cpp/rect_kernel_emu_head.inc (a shim: the lanes of a workgroup one after the other; the kernels have no
barrier) and rect_kernel_emu_tail.inc (the launch geometry) and compiled with the clang++ that hipcc drives. What this
checks without a GPU is the indexing, the tile and frame-group geometry, the tail-column and unaligned-row store paths and
the order of the fp64 operations as the host compiler takes them, and that no load of the remap kernel leaves the rows of
the source images (the shim counts such loads: emu_bad_loads); what it cannot check is the device's arithmetic and the
streams: that is tests/test_gpu_rectify.py. When a device test fails, the same case here separates an indexing bug (fails
here too) from a difference in the device's arithmetic (passes here)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as RC   # noqa: E402
from aria_slam_amd import rectify_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "rectify.hip")).read()
    body = src[src.index("\nnamespace {"):src.index("\n// ---- C-ABI")]
    assert "k_rect_build_map" in body and "k_rect_remap" in body and "k_rect_points" in body
    assert "asm" not in body, "the kernels are plain HIP C++"
    assert "__builtin_memcpy" in body, "the source loads (rect_ld_u16, rect_ld_u64) go through the name the shim checks"
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("rect_kernel_emu_head.inc", "rect_kernel_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "rect_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "rect_emu.cpp"), os.path.join(out_dir, "librect_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + parts[1])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, cpp])
    L = C.CDLL(so)
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.emu_build_map.argtypes = [p, i, i, i, i, p]
    L.emu_remap.argtypes = [p, i, i, p, i64, i, i, i, i, i, i, p, i64, i, i]
    L.emu_points.argtypes = [p, p, p, i64, i, p, p]
    L.emu_bad_loads.restype = C.c_long
    return L


def _cam_args(cam, new_K):
    return np.array(list(cam["K"]) + list(cam["dist"]) + list(cam["R"]) + list(new_K), np.float64)


def _aligned_words(n):
    raw = np.zeros(n * 4 + 64, np.uint8)
    off = (-raw.ctypes.data) % 16                                  # 16-byte aligned, as a device allocation is
    return raw[off:off + 4 * n].view(np.uint32)


def _emu_map(L, cam, new_K, dst, src=RC.SIZE):
    pitch = L.emu_map_pitch(dst[0])
    m = _aligned_words(pitch * dst[1])
    m[:] = 0x12345678
    a = _cam_args(cam, new_K)
    L.emu_build_map(a.ctypes.data, src[0], src[1], dst[0], dst[1], m.ctypes.data)
    return m, pitch


@pytest.fixture(scope="module")
def small_maps(emu):
    cl, cr, nk, _ = RC.cameras(RC.SMALL_NEW_K)
    return [_emu_map(emu, c, nk, RC.SMALL) for c in (cl, cr)]


@pytest.mark.parametrize("small", [False, True], ids=["752x480", "637x399"])
def test_map_kernel_source_is_bitwise_the_restatement(emu, small):
    """Shape (a). The padded columns of a map row are invalid."""
    cl, cr, nk, _ = RC.cameras(RC.SMALL_NEW_K if small else None)
    dst = RC.SMALL if small else RC.SIZE
    for k, cam in enumerate((cl, cr)):
        m, pitch = _emu_map(emu, cam, nk, dst)
        m = m.reshape(dst[1], pitch)
        want = RC.ref_maps(small)[k]
        assert m[:, :dst[0]].tobytes() == want.tobytes(), (small, k, int((m[:, :dst[0]] != want).sum()))
        assert (m[:, dst[0]:] == R.INVALID).all()
        share = (want == R.INVALID).mean()
        assert (0.10 < share < 0.30) if small else share < 0.01


def _emu_remap(L, m, frames, group, dst_pitch=RC.DST_PITCH, dst_stride=RC.DST_STRIDE, misalign=0, rows_ok=1):
    n = len(frames)
    src = RC.padded(frames, RC.SRC_PITCH, RC.SRC_STRIDE)
    raw = np.full(n * dst_stride + 8, 0x5A, np.uint8)
    dst = raw[misalign:misalign + n * dst_stride]
    L.emu_remap(m.ctypes.data, RC.SMALL[0], RC.SMALL[1], src.ctypes.data, RC.SRC_STRIDE, RC.SRC_PITCH, RC.SIZE[0], RC.SIZE[1], rows_ok,
                n, group, dst.ctypes.data, dst_stride, dst_pitch, RC.FILL)
    assert L.emu_bad_loads() == 0, "a load left the source images"
    img, is_pad = RC.unpadded(dst, n, RC.SMALL[1], RC.SMALL[0], dst_pitch, dst_stride)
    assert (dst.reshape(n, dst_stride)[is_pad] == 0x5A).all(), "padding was written"
    return img


def test_remap_kernel_source_is_bitwise_the_restatement(emu, small_maps):
    """Shape (b): five frames, uniform noise, pitched source with 0xA5 padding, odd destination pitch, fill = 7; with the
    shipped frame group, a group of 1, and a group of 2 (a last group of one frame); and with the per-pixel tap loads forced."""
    for k in range(2):
        want = RC.ref_remapped()[k]
        for group, rows_ok in ((emu.emu_group(), 1), (1, 1), (2, 1), (emu.emu_group(), 0)):
            got = _emu_remap(emu, small_maps[k][0], RC.noise_frames()[k], group, rows_ok=rows_ok)
            assert got.tobytes() == want.tobytes(), (k, group, rows_ok, int((got != want).sum()))
    assert (RC.ref_remapped() == RC.FILL).mean() > 0.10


def test_remap_kernel_source_batch_independence_and_alignments(emu, small_maps):
    """Shape (c): five frames in one call equal five calls of one frame; an aligned pitch (dword stores on every row) and a
    destination that starts at an odd address give the same pixels."""
    m = small_maps[0][0]
    frames = RC.noise_frames()[0]
    want = RC.ref_remapped()[0]
    for f in range(RC.N_FRAMES):
        assert _emu_remap(emu, m, frames[f:f + 1], emu.emu_group()).tobytes() == want[f:f + 1].tobytes(), f
    assert _emu_remap(emu, m, frames, emu.emu_group(), dst_pitch=640, dst_stride=640 * RC.SMALL[1]).tobytes() == want.tobytes()
    assert _emu_remap(emu, m, frames[:2], emu.emu_group(), misalign=1).tobytes() == want[:2].tobytes()


def test_points_kernel_source_is_bitwise_the_restatement(emu):
    """Shape (d): counts 0, 1 and kp_stride; in place equals out of place; a count of kp_stride + 1 skips its frame and
    raises the error bit."""
    kp, counts = RC.keypoints()
    cl, cr, nk, _ = RC.cameras(None)
    for k, cam in enumerate((cl, cr)):
        a = _cam_args(cam, nk)
        want = RC.ref_points(k, kp, counts)
        out = np.frombuffer(bytes([0x5A]) * kp.nbytes, np.uint8).copy().view(kp.dtype).reshape(kp.shape)
        err = np.zeros(1, np.int32)
        emu.emu_points(a.ctypes.data, kp.ctypes.data, counts.ctypes.data, RC.KP_STRIDE, 3, out.ctypes.data, err.ctypes.data)
        assert err[0] == 0
        for f, n in enumerate(counts):
            assert out[f, :n].tobytes() == want[f, :n].tobytes(), (k, f)
            assert (out[f, n:].view(np.uint8) == 0x5A).all()
        inplace = kp.copy()
        emu.emu_points(a.ctypes.data, inplace.ctypes.data, counts.ctypes.data, RC.KP_STRIDE, 3, inplace.ctypes.data, err.ctypes.data)
        assert inplace.tobytes() == want.tobytes() and err[0] == 0
        bad = np.array([RC.KP_STRIDE, RC.KP_STRIDE + 1, 1], np.int32)
        inplace = kp.copy()
        emu.emu_points(a.ctypes.data, inplace.ctypes.data, bad.ctypes.data, RC.KP_STRIDE, 3, inplace.ctypes.data, err.ctypes.data)
        assert err[0] == 1 and inplace.tobytes() == RC.ref_points(k, kp, bad).tobytes()
    assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()


# ---- the read forms, the frame groups and the limits (rectify_cases.EDGE_CASES) ---------------------------------------------
def _case_remap(L, case, m, frames, group, rows_ok=1, misalign=0):
    """The emulated kernel on a case's layouts -> the images; no padding byte written, no load outside the source images."""
    n = len(frames)
    src = case.src_buffer(frames)
    raw = np.full(n * case.dst_stride + 8, 0x5A, np.uint8)
    dst = raw[misalign:misalign + n * case.dst_stride]
    L.emu_remap(m.ctypes.data, case.dst[0], case.dst[1], src.ctypes.data, case.src_stride, case.src_pitch, case.src[0], case.src[1],
                rows_ok, n, group, dst.ctypes.data, case.dst_stride, case.dst_pitch, case.fill)
    bad = L.emu_bad_loads()
    assert bad == 0, "%s: %d loads left the source images" % (case.name, bad)
    img, pad_kept = case.images(dst, n)
    assert pad_kept, "padding was written"
    assert (raw[:misalign] == 0x5A).all() and (raw[misalign + n * case.dst_stride:] == 0x5A).all()
    return img


@pytest.fixture(scope="module")
def case_maps(emu):
    return {name: _emu_map(emu, c.cam, c.new_K, c.dst, c.src) for name, c in RC.EDGE_CASES.items() if name in RC.DEVICE_CASES}


@pytest.mark.parametrize("name", RC.DEVICE_CASES)
def test_edge_case_map_kernel_source_is_bitwise_the_restatement(case_maps, name):
    """k3 != 0, rotations far from the identity, Z <= 0 (yaw75), sources of 8x8 and 2x2, the 2047 limit with bit 31 set."""
    case = RC.EDGE_CASES[name]
    m, pitch = case_maps[name]
    m = m.reshape(case.dst[1], pitch)
    assert m[:, :case.dst[0]].tobytes() == case.map.tobytes(), (name, int((m[:, :case.dst[0]] != case.map).sum()))
    assert (m[:, case.dst[0]:] == R.INVALID).all()


@pytest.mark.parametrize("name", RC.DEVICE_CASES)
def test_edge_case_remap_kernel_source_is_bitwise_the_restatement(emu, case_maps, name):
    """Every frame of the case (17: groups of 8, 8 and 1) with the shipped group, with the tap loads forced, and with a group
    of 3 (the last group is short by one); frames 8 and 16, the first of the second group and the lone one of the third, in
    calls of their own; a destination at an odd address."""
    case = RC.EDGE_CASES[name]
    m = case_maps[name][0]
    for group, rows_ok in ((emu.emu_group(), 1), (emu.emu_group(), 0), (3, 1)):
        got = _case_remap(emu, case, m, case.frames, group, rows_ok)
        assert got.tobytes() == case.want.tobytes(), (name, group, rows_ok, int((got != case.want).sum()))
    for f in sorted({0, 8, 16} & set(range(case.n_frames))):
        assert _case_remap(emu, case, m, case.frames[f:f + 1], emu.emu_group()).tobytes() == case.want[f:f + 1].tobytes(), (name, f)
    assert _case_remap(emu, case, m, case.frames[:2], emu.emu_group(), misalign=1).tobytes() == case.want[:2].tobytes()
    src = case.src_buffer()
    dst = np.full(case.dst_stride, 0x5A, np.uint8)                                # no frame: nothing is read or written
    emu.emu_remap(m.ctypes.data, case.dst[0], case.dst[1], src.ctypes.data, case.src_stride, case.src_pitch, case.src[0], case.src[1],
                  1, 0, emu.emu_group(), dst.ctypes.data, case.dst_stride, case.dst_pitch, case.fill)
    assert (dst == 0x5A).all() and emu.emu_bad_loads() == 0


def test_edge_points_kernel_source_is_bitwise_the_restatement(emu):
    """NaN, infinite and huge keypoints, cameras that look away (Z <= 0): the (-1, -1) rule; in place equals out of place; a
    negative count skips its frame and raises the error bit."""
    kp, counts = RC.edge_keypoints(), RC.POINT_COUNTS
    for name, cam in RC.point_cameras():
        want = RC.ref_edge_points_all()[name][0]
        a = _cam_args(cam, cam["K"])
        out = np.frombuffer(bytes([0x5A]) * kp.nbytes, np.uint8).copy().view(kp.dtype).reshape(kp.shape)
        err = np.zeros(1, np.int32)
        emu.emu_points(a.ctypes.data, kp.ctypes.data, counts.ctypes.data, RC.KP_STRIDE, 2, out.ctypes.data, err.ctypes.data)
        assert err[0] == 0
        for f, n in enumerate(counts):
            assert out[f, :n].tobytes() == want[f, :n].tobytes(), (name, f)
            assert (out[f, n:].view(np.uint8) == 0x5A).all()
        inplace = kp.copy()
        emu.emu_points(a.ctypes.data, inplace.ctypes.data, counts.ctypes.data, RC.KP_STRIDE, 2, inplace.ctypes.data, err.ctypes.data)
        assert inplace.tobytes() == want.tobytes() and err[0] == 0
        bad = np.array([-1, RC.KP_STRIDE], np.int32)
        inplace = kp.copy()
        emu.emu_points(a.ctypes.data, inplace.ctypes.data, bad.ctypes.data, RC.KP_STRIDE, 2, inplace.ctypes.data, err.ctypes.data)
        assert err[0] == 1 and inplace[0].tobytes() == kp[0].tobytes()
        assert inplace.tobytes() == RC.ref_edge_points(cam, kp, bad).tobytes()
