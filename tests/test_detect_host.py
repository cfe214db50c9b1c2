"""The object-detector stage without a GPU: known answers of the restatement (aria_slam_amd/detect_ref.py, the definition the
kernels are held to bitwise in tests/test_gpu_detect.py), worked by hand here; the aria_det_* family's ABI; and the C++
adapter's build.

The hand-worked resize values follow from the coefficient rule alone. For a 2x upscale of a 2-pixel axis the source
position of destination d is (d + 0.5) * 0.5 - 0.5 = -0.25, 0.25, 0.75, 1.25: the first is clamped to pixel 0, the last to
pixel 1, the middle two weigh the second pixel with cvRound(0.25 * 2048) = 512 and cvRound(0.75 * 2048) = 1536 of 2048."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aria_slam_amd import detect_ref as R
from detect_cases import POST_CASES, build_selftest, run_case_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")

DET_SYMBOLS = ["aria_det_default_config", "aria_det_create", "aria_det_destroy", "aria_det_check", "aria_det_stream",
               "aria_det_device_buffers", "aria_det_preprocess_batch_device", "aria_det_postprocess_batch_device",
               "aria_det_preprocess", "aria_det_postprocess", "aria_det_resize_table", "aria_det_algorithmic_bytes"]


def _vert(s0, s1, b1):
    return (((2048 - b1) * (s0 >> 4) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2


# ---- resize
def test_identity_resize_returns_the_input():
    rng = np.random.default_rng(1)
    for shape in ((7, 5), (16, 16), (9, 11, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(R.resize_linear_u8(img, shape[1], shape[0]), img)


def test_2x_upscale_of_a_2x2_image_by_hand():
    img = np.array([[0, 100], [200, 40]], np.uint8)
    x0, x1, a = R.resize_table(2, 4)
    assert x0.tolist() == [0, 0, 0, 1] and x1.tolist() == [1, 1, 1, 1] and a.tolist() == [0, 512, 1536, 0]
    # horizontal pass, in 1/2048: p0 * (2048 - a) + p1 * a
    top = [0 * 2048, 0 * 1536 + 100 * 512, 0 * 512 + 100 * 1536, 100 * 2048]
    bot = [200 * 2048, 200 * 1536 + 40 * 512, 200 * 512 + 40 * 1536, 40 * 2048]
    want = [[_vert(t, b, b1) for t, b in zip(top, bot)] for b1 in (0, 512, 1536)] + [[_vert(b, b, 0) for b in bot]]
    assert want == [[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55], [200, 160, 80, 40]]   # the same, written out
    assert R.resize_linear_u8(img, 4, 4).tolist() == want


def test_a_constant_image_stays_constant_at_any_ratio():
    for v in (0, 1, 127, 200, 255):
        img = np.full((23, 37), v, np.uint8)
        for w, h in ((16, 12), (37, 23), (80, 51), (5, 90), (1, 1)):
            assert (R.resize_linear_u8(img, w, h) == v).all(), (v, w, h)


def test_both_border_clamps():
    x0, x1, a = R.resize_table(5, 16)
    assert x0[0] == 0 and a[0] == 0 and x0[-1] == 4 and x1[-1] == 4 and a[-1] == 0
    assert (x0 >= 0).all() and (x1 <= 4).all() and (a >= 0).all() and (a <= 2048).all()
    x0, x1, a = R.resize_table(37, 16)                       # downscale: no clamp on the left, taps stay inside
    assert x0[0] == 0 and a[0] > 0 and x1.max() <= 36


# ---- planes
def test_gray_gives_three_equal_planes_and_scale_is_one_multiply():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 9, 13), dtype=np.uint8)
    out = R.preprocess_ref(img, 13, 9, 1, True)
    assert out.shape == (2, 3, 9, 13) and out.dtype == np.float32
    want = img.astype(np.float32) * np.float32(1.0 / 255.0)
    for p in range(3):
        assert out[:, p].tobytes() == want.tobytes()
    assert out.max() <= 1.0


def test_swap_rb_exchanges_planes_0_and_2():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (1, 10, 12, 3), dtype=np.uint8)
    a, b = R.preprocess_ref(img, 8, 6, 3, False), R.preprocess_ref(img, 8, 6, 3, True)
    assert np.array_equal(a[:, 0], b[:, 2]) and np.array_equal(a[:, 2], b[:, 0]) and np.array_equal(a[:, 1], b[:, 1])
    assert a[0, 0].tobytes() == R.preprocess_ref(np.ascontiguousarray(img[..., 0]), 8, 6, 1)[0, 0].tobytes()


def test_half_output_is_float16_of_the_float_output():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (1, 10, 12, 3), dtype=np.uint8)
    f, h = R.preprocess_ref(img, 8, 6, 3, True), R.preprocess_ref(img, 8, 6, 3, True, half=True)
    assert h.dtype == np.float16 and h.tobytes() == f.astype(np.float16).tobytes()


# ---- postprocess: the case table of tests/detect_cases.py (tests/test_gpu_detect.py runs it through the device)
@pytest.mark.parametrize("name", sorted(POST_CASES))
def test_postprocess_known_answers(name):
    raw, _, want, n_dyn = POST_CASES[name]
    dets, boxes = run_case_ref(name)
    got = [(float(d["x1"]), float(d["y1"]), float(d["x2"]), float(d["y2"]), int(d["class_id"])) for d in dets]
    assert got == [tuple(float(v) for v in w[:4]) + (w[4],) for w in want]
    assert len(boxes) == n_dyn
    assert dets.dtype.itemsize == 24 and boxes.dtype.itemsize == 16
    # the confidence is the candidate's own float, untouched, and the order is descending
    assert all(np.float32(c) in raw[:, 4] for c in dets["confidence"])
    assert (np.diff(dets["confidence"]) <= 0).all()
    # the dynamic boxes are the detections' corners, in their order
    if name == "dynamic_subset":
        assert boxes.tolist() == [(20.0, 0.0, 30.0, 10.0), (60.0, 0.0, 70.0, 10.0)]


def test_overlap_is_fp64_division_then_one_fp32_rounding():
    # 10x10 boxes shifted by 4: intersection 60, union 140
    ov = R.rect_overlap((0, 0, 10, 10), (4, 0, 14, 10))
    assert ov.dtype == np.float32 and ov == np.float32(1.0) - np.float32(1.0 - 60.0 / 140.0)
    assert R.rect_overlap((0, 0, 10, 10), (10, 0, 20, 10)) == 0.0
    assert R.rect_overlap((5, 5, 5, 9), (50, 50, 58, 50)) == 1.0
    # exact areas (divergence D2): 2^20-sided squares do not overflow
    big = (0, 0, 2 ** 20, 2 ** 20)
    assert R.rect_overlap(big, big) == 1.0


# ---- ABI and build
def test_det_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", aria.library_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in DET_SYMBOLS:
        assert name in exported, name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    declared = {n for n in DET_SYMBOLS if (n + "(") in header}
    assert declared == set(DET_SYMBOLS)
    assert aria.abi_version() == 4 and "#define ARIA_ORB_HIP_ABI_VERSION 4" in header


def test_det_record_layouts_and_defaults(aria, tmp_path):
    from aria_slam_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "aria_orb_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(aria_detection), '
                   'sizeof(aria_box), sizeof(aria_det_config)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert sizes == [24, 16, C.sizeof(_lib.DetConfig)] and _lib.DETECTION_DTYPE.itemsize == 24 and _lib.BOX_DTYPE.itemsize == 16
    assert _lib.DETECTION_DTYPE == R.DETECTION_DTYPE and _lib.BOX_DTYPE == R.BOX_DTYPE
    cfg = _lib.DetConfig()
    aria.load_library().aria_det_default_config(C.byref(cfg))
    assert (cfg.struct_size, cfg.input_w, cfg.input_h, cfg.max_batch, cfg.max_candidates, cfg.out_half) == (sizes[2], 640, 640, 1, 300, 0)


def test_argument_errors_are_status_codes_before_any_device_is_touched(aria):
    """What can be refused without a handle is refused with ARIA_E_INVALID whether or not a GPU is present; a valid
    configuration then fails loudly with ARIA_E_NO_DEVICE where there is none (the handle-level argument errors are in
    tests/test_gpu_detect.py)."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    h = C.c_void_p()

    def create(**kw):
        cfg = _lib.DetConfig()
        L.aria_det_default_config(C.byref(cfg))
        for k, v in kw.items():
            setattr(cfg, k, v)
        return L.aria_det_create(C.byref(cfg), C.byref(h))

    for bad in ({"struct_size": 8}, {"max_candidates": 1025}, {"max_candidates": 0}, {"input_w": 0}, {"input_h": -5}, {"max_batch": 0},
                {"out_half": 2}, {"input_w": 1 << 20}):
        assert create(**bad) == -1, bad
        assert not h.value
    assert L.aria_det_create(None, C.byref(h)) == -1
    assert L.aria_det_check(None, None, None) == -1
    assert L.aria_det_preprocess_batch_device(None, None, 1, 16, 16, 16, 256, 1, 0, None) == -1
    assert L.aria_det_postprocess_batch_device(None, None, 1, 300, 16, 16, 0.5, 0.45, None, 0, None, None, 0, None, None, 0) == -1
    L.aria_det_destroy(None)
    import torch
    if not torch.cuda.is_available():
        assert create() == -2                                    # ARIA_E_NO_DEVICE
        assert "no usable HIP device" in aria.status_string(-2)
        with pytest.raises(aria.AriaError):
            aria.HipObjectDetector()


def test_resize_table_of_the_library_is_the_restatements(aria):
    from aria_slam_amd import detect
    for src, dst in ((37, 16), (23, 12), (5, 16), (7, 16), (16, 16), (16, 18), (752, 640), (480, 640), (1, 7), (9, 1), (4000, 333)):
        x0, _, a = R.resize_table(src, dst)
        t0, ta = detect.resize_table(src, dst)
        assert np.array_equal(x0, t0) and np.array_equal(a, ta), (src, dst)
    L = aria.load_library()
    assert L.aria_det_algorithmic_bytes(752, 480, 1, 640, 640, 0) == 752 * 480 + 3 * 640 * 640 * 4
    assert L.aria_det_algorithmic_bytes(752, 480, 3, 640, 640, 1) == 752 * 480 * 3 + 3 * 640 * 640 * 2
    buf = np.zeros(4, np.uint32)
    assert L.aria_det_resize_table(16, 8, buf.ctypes.data, 4) == -1           # capacity
    assert L.aria_det_resize_table(0, 8, buf.ctypes.data, 4) == -1


def test_detect_stage_is_in_the_product_build_without_float_atomics_or_environment():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "detect_stage.hip" in mk.split("SRC :=")[1].split("\n")[0]
    text = open(os.path.join(PKG, "csrc", "detect_stage.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    text += "".join(open(os.path.join(PKG, "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in text)
    assert "getenv" not in text and "atomicAdd(&s_m" in text
    for line in text.splitlines():
        if "atomic" in line and not line.lstrip().startswith("//"):
            assert "float" not in line and "double" not in line, line


def test_det_selftest_compiles_links_and_fails_loudly_without_gpu(aria):
    exe = build_selftest()
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True).stdout
    for name in ("aria::adapters::hip::makeObjectDetector", "aria::factory::createHipDetector"):
        assert name in syms, name
    import torch
    if torch.cuda.is_available():
        return                                                   # the GPU half of the selftest is tests/test_gpu_detect.py
    out = subprocess.run([exe, "nogpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK nogpu" in out.stdout and "no usable HIP device" in out.stdout
