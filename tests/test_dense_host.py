"""Dense stereo (include/aria_orb_hip.h, "dense stereo"): the parts that need no GPU -- exports, the config's layout, defaults
and validation, the NumPy restatement (aria_slam_amd/dense_ref.py, which is the definition) on hand-made known answers,
the sub-pixel rule, its accuracy on the synthetic rectified scene, and the kernels' listing."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_kernel_stats as S   # noqa: E402
import dense_cases as DC   # noqa: E402

DENSE_SYMBOLS = ["aria_dense_default_config", "aria_dense_create", "aria_dense_destroy", "aria_dense_stream", "aria_dense_check",
                 "aria_dense_compute_batch_device", "aria_dense_compute", "aria_dense_sample_batch_device", "aria_dense_sample",
                 "aria_dense_pairs_in_flight", "aria_dense_scratch_bytes_per_pair", "aria_dense_algorithmic_bytes"]
KERNELS = ("k_dense_census", "k_dense_horiz", "k_dense_down", "k_dense_up_win", "k_dense_finish", "k_dense_sample")


def test_dense_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in DENSE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipDenseStereo" in aria.__all__
    assert re.search(r"#define\s+ARIA_DENSE_NO_KEYPOINT\s+0x7FFFFFFF", header) and _lib.DENSE_NO_KEYPOINT == 0x7FFFFFFF


def test_dense_config_layout_and_defaults(aria):
    from aria_slam_amd import _lib, dense_ref
    L = aria.load_library()
    assert C.sizeof(_lib.DenseConfig) == 96
    cfg = _lib.DenseConfig()
    L.aria_dense_default_config(C.byref(cfg))
    assert cfg.struct_size == 96 and not cfg.stream
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.baseline) == (458.654, 457.296, 367.215, 248.375, 0.110)
    assert (cfg.num_disparities, cfg.P1, cfg.P2, cfg.uniqueness, cfg.lr_max_diff) == (64, 8, 32, 10, 1)
    assert (cfg.max_width, cfg.max_height, cfg.scratch_bytes) == (752, 480, 1 << 30)
    d = dense_ref.DEFAULTS
    assert (d["baseline"], d["P1"], d["P2"], d["uniqueness"], d["lr_max_diff"], dense_ref.D) == (0.110, 8, 32, 10, 1, 64)
    assert L.aria_dense_scratch_bytes_per_pair(640, 480) == 148 * 640 * 480 == dense_ref.scratch_bytes_per_pair(640, 480)
    assert L.aria_dense_algorithmic_bytes(640, 480) == 8 * 640 * 480
    assert L.aria_dense_pairs_in_flight(None) == -1 and L.aria_dense_check(None) == -1


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("fx", 0.0), ("fy", float("nan")), ("baseline", 0.0),
                                         ("num_disparities", 128), ("num_disparities", 32), ("P1", 0), ("P1", 33), ("P2", 128),
                                         ("uniqueness", -1), ("uniqueness", 100), ("lr_max_diff", 64), ("max_width", 0),
                                         ("max_width", 4097), ("max_height", 4097), ("scratch_bytes", 0),
                                         ("scratch_bytes", 148 * 752 * 480 - 1)])
def test_dense_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched: only 64 disparities, 1 <= P1 <= P2 <= 127, and a scratch
    budget that holds at least one pair of max_width x max_height."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.DenseConfig()
    L.aria_dense_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_dense_create(C.byref(cfg), C.byref(h)) == -1       # ARIA_E_INVALID
    assert not h.value
    assert L.aria_dense_create(None, C.byref(h)) == -1


def test_dense_calls_refuse_null_handles(aria):
    L = aria.load_library()
    assert L.aria_dense_compute_batch_device(None, None, None, 0, 64, 8, 64, 1, None, 0, 64, None, 0, 64) == -1
    assert L.aria_dense_compute(None, None, None, 64, 8, 64, None, None) == -1
    assert L.aria_dense_sample_batch_device(None, None, 0, 64, 64, 8, None, None, 4, 1, None) == -1
    assert L.aria_dense_sample(None, None, 64, 8, 64, None, 0, None) == -1
    assert L.aria_dense_stream(None) is None


def test_no_gpu_means_dense_create_fails_loudly(aria):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(aria.AriaError) as e:
        aria.HipDenseStereo()
    assert e.value.status == -2                                      # ARIA_E_NO_DEVICE: there is no CPU fallback


def test_ref_shifted_pair_gives_the_shift():
    """The right image is the left one moved by exactly 5 px: the winner is d = 5 at every pixel away from the borders
    (x >= 64 + 5 keeps every disparity's right pixel inside; the last 5 + 4 columns see the replicated edge), C(5) = 0 there,
    and d16 lies within rule 7's reach of 80, [80 - 7, 80 + 8]. d16 is exactly 80 only where S(4) and S(6) balance
    (-1 < 8 (S(4) - S(6)) / den2 + 0.5 < 1): the sums of the two wrong neighbours are noise on any texture (uniform noise,
    the rectangle scene and smoothed noise all give 52-53 % exactly 80, the rest 75..87), so rule 7 moves the other pixels
    by a few sixteenths. The depth at exactly 80 is fb / 5."""
    from aria_slam_amd import dense_ref as R
    rng = np.random.default_rng(5)
    W, H = 160, 24
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = np.empty_like(left)
    right[:, :W - 5] = left[:, 5:]
    right[:, W - 5:] = left[:, -1:]
    d16 = R.dense_disparity(left, right)
    assert d16.dtype == np.int16 and d16.shape == (H, W)
    inner = d16[:, 69:W - 9]
    print("exactly 80: %.4f, range %d..%d" % ((inner == 80).mean(), inner.min(), inner.max()))
    assert ((inner + 7) >> 4 == 5).all() and (inner >= 73).all() and (inner <= 88).all()
    assert (inner == 80).mean() > 0.5
    assert (R.sgm_volume(left, right)[:, 69:W - 9].argmin(axis=2) == 5).all()
    z = R.depth_map(d16)
    fb = np.float32(458.654) * np.float32(0.110)
    assert z.dtype == np.float32 and (z[d16 == 80] == fb / np.float32(5.0)).all()
    assert (z[d16 <= 0] == 0).all() and np.isfinite(z).all()
    # the cost itself: zero at d = 5, and the constant 64 where x - d < 0
    cen_l, cen_r = R.census(left), R.census(right)
    Cv = R.cost_volume(cen_l, cen_r)
    assert (Cv[:, 69:W - 9, 5] == 0).all() and (Cv[:, 3, 4:] == 64).all() and Cv[:, 3, :4].max() <= 62
    assert int(cen_l.max()) < (1 << 62)                              # 62 neighbours


def test_ref_constant_pair():
    """Every census word is 0, so C = 0 where x - d >= 0 and 64 elsewhere. S(0) = 0 is the least sum everywhere and d = 0 the
    lowest index that reaches it: best = 0. Uniqueness compares S(d) * 90 < 0: never. The right view's minimum is 0 at
    d = 0 as well, so the left-right check passes. best = 0 takes no sub-pixel step: d16 = 0 on every pixel, depth 0."""
    from aria_slam_amd import dense_ref as R
    left, right = DC.const_pair()
    S_ = R.sgm_volume(left, right)
    assert (S_[:, :, 0] == 0).all() and S_.min() == 0
    d16 = R.dense_disparity(left, right)
    assert (d16 == 0).all()
    assert (R.depth_map(d16) == 0).all()
    assert (R.dense_disparity(left, right, lr_max_diff=-1, uniqueness=99) == 0).all()


def test_ref_aggregation_by_hand():
    """A one-row pair: only the two horizontal paths move, the vertical ones add C twice. Checked against a direct
    per-pixel loop of rule 3."""
    from aria_slam_amd import dense_ref as R
    rng = np.random.default_rng(11)
    Cv = rng.integers(0, 63, (1, 7, 64)).astype(np.uint8)
    P1, P2 = 3, 9
    want = 2 * Cv[0].astype(np.int64)
    for order in (range(7), range(6, -1, -1)):
        prev = None
        for x in order:
            c = Cv[0, x].astype(np.int64)
            if prev is None:
                L = c.copy()
            else:
                m = prev.min()
                L = np.empty(64, np.int64)
                for d in range(64):
                    cand = [prev[d], m + P2]
                    if d > 0:
                        cand.append(prev[d - 1] + P1)
                    if d < 63:
                        cand.append(prev[d + 1] + P1)
                    L[d] = c[d] + min(cand) - m
            want[x] += L
            prev = L
    assert np.array_equal(R.aggregate(Cv, P1, P2)[0], want)


def test_ref_subpixel_rule():
    from aria_slam_amd import dense_ref as R
    assert R.subpixel(10, 5, 10, 7) == 112                           # symmetric: (0 + 10) / 20 truncates to 0
    assert R.subpixel(20, 5, 10, 7) == 116                           # (160 + 20) / 40 = 4.5 -> 4
    assert R.subpixel(10, 5, 20, 7) == 109                           # (-160 + 20) / 40 = -3.5 -> -3: towards zero, not floor (-4)
    assert R.subpixel(5, 5, 5, 7) == 112                             # den2 = 0 clamped to 1: (0 + 1) / 2 = 0
    assert R.subpixel(6, 5, 4, 7) == 112 + 16                        # den2 = 0 clamped to 1: (32 + 1) / 2 = 16
    assert R.subpixel(4, 5, 6, 7) == 112 - 15                        # den2 = 0 clamped to 1: (-32 + 1) / 2 = -15.5 -> -15
    # the map applies the same rule, and none at best = 0 and best = 63
    S_ = np.full((1, 3, 64), 500, np.int32)
    S_[0, 0, 6:9] = (10, 5, 20)
    S_[0, 1, 0:2] = (5, 9)
    S_[0, 2, 62:64] = (9, 5)
    d16 = R.disparity_from_volume(S_, uniqueness=0, lr_max_diff=-1)
    assert list(d16[0]) == [109, 0, 16 * 63]


def test_ref_uniqueness_and_left_right_rules():
    from aria_slam_amd import dense_ref as R
    S_ = np.full((1, 80, 64), 500, np.int32)
    S_[0, 70, 10] = 100
    S_[0, 70, 30] = 111                                              # 111 * 90 = 9990 < 10000: ambiguous
    S_[0, 71, 10] = 100
    S_[0, 71, 30] = 112                                              # 112 * 90 = 10080: unique
    S_[0, 72, 10] = 100
    S_[0, 72, 11] = 100                                              # the neighbour of the winner does not count; tie -> d = 10
    S_[0, 5, 10] = 100                                               # x - best < 0
    d = R.disparity_from_volume(S_, uniqueness=10, lr_max_diff=-1)
    assert d[0, 70] == -16 and d[0, 71] > 0 and (d[0, 71] + 7) >> 4 == 10 and (d[0, 72] + 7) >> 4 == 10 and (d[0, 5] + 7) >> 4 == 10
    assert R.disparity_from_volume(S_, uniqueness=0, lr_max_diff=-1)[0, 70] > 0
    # left-right: pixel 5 has no right pixel; right pixel 61 is claimed by x = 71 (d = 10) and, better, by x = 73 (d = 12)
    S_[0, 73, 12] = 50
    assert R.right_disparity(S_)[0, 61] == 12
    d = R.disparity_from_volume(S_, uniqueness=0, lr_max_diff=1)
    assert d[0, 5] == -16 and d[0, 71] == -16 and d[0, 73] > 0
    d = R.disparity_from_volume(S_, uniqueness=0, lr_max_diff=2)
    assert d[0, 71] > 0


@pytest.mark.parametrize("W,H", DC.ACCURACY_SHAPES, ids=["200x96", "320x240"])
@pytest.mark.parametrize("seed", DC.SCENE_SEEDS)
def test_ref_accuracy_on_the_synthetic_scene(seed, W, H):
    """stereo_ref.stereo_pair (row disparities 7.0, 19.5, 42.25), default parameters, over the columns x >= 64. Measured
    with this restatement: valid share 0.9917 / 0.9936 (200x96, seeds 1 / 2) and 0.9970 / 0.9950 (320x240); of the valid
    pixels 0.9790 / 0.9799 and 0.9826 / 0.9817 within 0.5 px, 0.9986 / 0.9989 and 0.9998 / 0.9995 within 1 px."""
    left, right, truth = DC.scene_pair(seed, W, H)
    d16, z = DC.ref(left, right)
    sub = d16[:, 64:].astype(np.float64) / 16.0
    valid = d16[:, 64:] > 0
    err = np.abs(sub - truth[:, None])[valid]
    print("seed %d %dx%d: valid %.4f, within 0.5 px %.4f, within 1 px %.4f"
          % (seed, W, H, valid.mean(), (err <= 0.5).mean(), (err <= 1.0).mean()))
    assert valid.mean() >= 0.95
    assert (err <= 0.5).mean() >= 0.95
    assert (err <= 1.0).mean() >= 0.99
    assert np.isfinite(z).all() and (z[d16 > 0] > 0).all() and (z[d16 <= 0] == 0).all()


def test_ref_sampling_rules():
    from aria_slam_amd import dense_ref as R
    from aria_slam_amd import stereo_ref
    from aria_slam_amd._lib import KP_DTYPE
    d16 = np.full((4, 6), -16, np.int16)
    d16[0, 2] = 80
    d16[2, 4] = 0
    kp = np.zeros(6, KP_DTYPE)
    kp["x"] = [2.5, 3.5, 4.0, -0.6, 5.6, np.nan]                     # rint: 2 (half to even), 4, 4, -1, 6
    kp["y"] = [0.5, 0.0, 2.0, 0.0, 0.0, 0.0]                         # rint: 0 (half to even)
    obs = R.sample(d16, kp)
    none = stereo_ref.unmatched_obs(1)[0]
    assert all(obs[i] == none for i in (1, 2, 3, 4, 5))              # invalid pixel, d16 = 0, outside twice, NaN
    fx, fy, cx, cy = (np.float32(v) for v in R.EUROC_K)
    depth = fx * np.float32(0.110) / np.float32(5.0)
    o = obs[0]
    assert (o["disparity"], o["depth"], o["u_right"]) == (np.float32(5.0), depth, np.float32(-2.5))
    assert o["X"] == (np.float32(2.5) - cx) * depth / fx and o["Y"] == (np.float32(0.5) - cy) * depth / fy
    assert (o["right_idx"], o["hamming"], o["sad"]) == (0x7FFFFFFF, 0, 0)
    # the batch form: beyond the count and a count out of range
    b = R.sample_batch([d16, d16], np.stack([kp, kp]), [1, 7])
    assert b[0, 0] == o and all(b[0, i] == none for i in range(1, 6)) and all(b[1, i] == none for i in range(6))


def test_dense_kernels_cross_compile_without_scratch():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "dense_stereo.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "dense_stereo.hip")])
    text = open(path).read()
    for k in KERNELS:
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        hist, _, _ = S.stats(body)
        assert not any(op.startswith("global_atomic") and ("f32" in op or "f64" in op) for op in hist), k   # no float atomics
    for k in ("k_dense_horiz", "k_dense_down", "k_dense_up_win"):
        hist, _, _ = S.stats(S.kernel_body(text, k)[0])
        assert hist["v_bcnt_u32_b32"] >= 2, k                                     # the cost: popcount of two census words
        assert sum(n for op, n in hist.items() if op.endswith("_dpp")) >= 8, k    # lane shifts and the wave reduction
        assert not any(op.startswith(("ds_bpermute", "ds_permute", "ds_swizzle")) for op in hist), k
    hist, _, _ = S.stats(S.kernel_body(text, "k_dense_up_win")[0])
    assert hist["global_atomic_umin"] >= 1                           # the right view's packed minimum
    # correctly rounded divisions: the depth; the sampled depth, X and Y (their v_fma_f32 are the division's own steps)
    assert S.stats(S.kernel_body(text, "k_dense_finish")[0])[0]["v_div_fixup_f32"] == 1
    assert S.stats(S.kernel_body(text, "k_dense_sample")[0])[0]["v_div_fixup_f32"] == 3


def test_dense_stereo_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "dense_stereo.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "dense_stereo.hip")).read()
    src += open(os.path.join(ROOT, "aria_slam_amd", "csrc", "stage_handle.h")).read()
    assert "getenv" not in src
