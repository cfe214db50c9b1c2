"""Dense depth fusion (include/aria_orb_hip.h, "dense depth fusion"): the parts that need no GPU -- exports, the layouts,
defaults and validation, the NumPy restatement (aria_slam_amd/tsdf_ref.py, which is the definition) against a plain
per-voxel loop and on known answers, its accuracy on the analytic scene, and the kernels' listing."""
import ctypes as C
import math
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
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import tsdf_ref as R   # noqa: E402

TSDF_SYMBOLS = ["aria_tsdf_default_config", "aria_tsdf_create", "aria_tsdf_destroy", "aria_tsdf_stream", "aria_tsdf_check",
                "aria_tsdf_clear", "aria_tsdf_integrate_batch_device", "aria_tsdf_integrate", "aria_tsdf_extract_points_device",
                "aria_tsdf_extract_points", "aria_tsdf_device_voxels", "aria_tsdf_read_box", "aria_tsdf_volume_bytes",
                "aria_tsdf_algorithmic_bytes"]
KERNELS = ("k_tsdf_prepare", "k_tsdf_cull", "k_tsdf_integrate", "k_tsdf_count", "k_tsdf_scan", "k_tsdf_emit")
f32 = np.float32


def test_tsdf_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in TSDF_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipTsdfVolume" in aria.__all__


def test_tsdf_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    assert C.sizeof(_lib.TsdfConfig) == 104
    assert _lib.TSDF_VOXEL_DTYPE.itemsize == 8 == R.VOXEL_DTYPE.itemsize and _lib.TSDF_VOXEL_DTYPE == R.VOXEL_DTYPE
    assert _lib.TSDF_POINT_DTYPE.itemsize == 16 == R.POINT_DTYPE.itemsize and _lib.TSDF_POINT_DTYPE == R.POINT_DTYPE
    cfg = _lib.TsdfConfig()
    L.aria_tsdf_default_config(C.byref(cfg))
    assert cfg.struct_size == 104 and not cfg.stream
    assert (cfg.nx, cfg.ny, cfg.nz, cfg.max_weight, cfg.min_weight) == (256, 256, 128, 64, 2)
    assert (cfg.voxel, cfg.trunc, cfg.min_depth, cfg.max_depth) == (f32(0.05), f32(0.20), f32(0.3), f32(10.0))
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375)
    d = R.config()
    assert d.dims == (256, 256, 128) and (d.voxel, d.trunc, d.min_depth, d.max_depth) == (cfg.voxel, cfg.trunc, cfg.min_depth, cfg.max_depth)
    assert tuple(d.origin) == tuple(f32(v) for v in cfg.origin) and (d.max_weight, d.min_weight) == (64, 2) and d.K == R.EUROC_K
    assert L.aria_tsdf_volume_bytes(256, 256, 128) == 64 << 20 == R.volume_bytes(256, 256, 128)
    assert L.aria_tsdf_volume_bytes(12, 8, 8) == -1 and L.aria_tsdf_volume_bytes(8, 8, 1032) == -1
    assert L.aria_tsdf_algorithmic_bytes(256, 256, 128, 752, 480, 32) == 16 * 256 * 256 * 128 + 4 * 752 * 480 * 32
    assert R.algorithmic_bytes(256, 256, 128, 752, 480, 32) == L.aria_tsdf_algorithmic_bytes(256, 256, 128, 752, 480, 32)
    assert L.aria_tsdf_check(None) == -1 and L.aria_tsdf_clear(None) == -1


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("nx", 12), ("ny", 0), ("nz", 1032), ("nz", 4), ("voxel", 0.0),
                                         ("voxel", float("nan")), ("trunc", 0.0), ("trunc", -1.0), ("min_depth", 11.0),
                                         ("max_depth", float("nan")), ("max_weight", 0), ("max_weight", 65536), ("min_weight", 0),
                                         ("min_weight", 65536), ("fx", float("inf"))])
def test_tsdf_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched, and the restatement refuses the same."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.TsdfConfig()
    L.aria_tsdf_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_tsdf_create(C.byref(cfg), C.byref(h)) == -1        # ARIA_E_INVALID
    assert not h.value
    assert L.aria_tsdf_create(None, C.byref(h)) == -1
    if field in ("nx", "ny", "nz"):
        dims = {"nx": 256, "ny": 256, "nz": 128}
        dims[field] = value
        with pytest.raises(ValueError):
            R.config(dims=(dims["nx"], dims["ny"], dims["nz"]))
    elif field not in ("struct_size", "fx"):
        with pytest.raises(ValueError):
            R.config(**{field: value})


def test_tsdf_calls_refuse_null_handles(aria):
    L = aria.load_library()
    assert L.aria_tsdf_integrate_batch_device(None, None, 0, 8, 8, 8, None, None, None, 0, 8, 1) == -1
    assert L.aria_tsdf_integrate(None, None, 8, 8, 8, None, None, 0) == -1
    assert L.aria_tsdf_extract_points_device(None, None, 0, None) == -1
    assert L.aria_tsdf_extract_points(None, None, 0, None) == -1
    assert L.aria_tsdf_read_box(None, 0, 0, 0, 1, 1, 1, None) == -1
    assert L.aria_tsdf_stream(None) is None and L.aria_tsdf_device_voxels(None) is None


def test_no_gpu_means_tsdf_create_fails_loudly(aria):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(aria.AriaError) as e:
        aria.HipTsdfVolume(dims=(8, 8, 8))
    assert e.value.status == -2                                      # ARIA_E_NO_DEVICE: there is no CPU fallback


def _loop_integrate(vol, cfg, depth, ext, image):
    """Rules 3a-3h for one frame, voxel by voxel, in NumPy fp32 scalars."""
    e = np.asarray(ext, np.float64).astype(f32)
    Hh, Ww = depth.shape
    fx, fy, cx, cy = (f32(v) for v in cfg.K)
    inv_trunc = f32(1.0) / cfg.trunc
    nx, ny, nz = cfg.dims
    one, half = f32(1.0), f32(0.5)
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    cX = cfg.origin[0] + (f32(i) + half) * cfg.voxel
                    cY = cfg.origin[1] + (f32(j) + half) * cfg.voxel
                    cZ = cfg.origin[2] + (f32(k) + half) * cfg.voxel
                    xc = ((e[0] * cX + e[1] * cY) + e[2] * cZ) + e[3]
                    yc = ((e[4] * cX + e[5] * cY) + e[6] * cZ) + e[7]
                    zc = ((e[8] * cX + e[9] * cY) + e[10] * cZ) + e[11]
                    if not zc >= cfg.min_depth:
                        continue
                    iz = one / zc
                    u = (fx * xc) * iz + cx
                    v = (fy * yc) * iz + cy
                    ur, vr = np.rint(u), np.rint(v)
                    if not (0 <= ur <= f32(Ww - 1) and 0 <= vr <= f32(Hh - 1)):
                        continue
                    ui, vi = int(ur), int(vr)
                    D = depth[vi, ui]
                    if not (D >= cfg.min_depth and D <= cfg.max_depth):
                        continue
                    sdf = D - zc
                    if sdf < -cfg.trunc:
                        continue
                    s = min(one, sdf * inv_trunc)
                    rec = vol[k, j, i]
                    W0 = int(rec["weight"])
                    w = f32(W0)
                    rec["tsdf"] = (rec["tsdf"] * w + s) / (w + one)
                    if image is not None:
                        rec["gray"] = (int(rec["gray"]) * W0 + int(image[vi, ui]) + ((W0 + 1) >> 1)) // (W0 + 1)
                    rec["weight"] = min(W0 + 1, cfg.max_weight)


def test_ref_equals_a_plain_per_voxel_loop():
    """The vectorised restatement against rules 3a-3h written as a loop, on shape (b): 8 x 8 x 8 voxels, three frames whose
    5 x 3 depth maps hold every kind of bad value, with and without images."""
    cfg, want, _ = TC.ref_small()
    d, im, e = TC.small_frames()
    for images in (im, None):
        vol = R.new_volume(cfg)
        for f in range(3):
            _loop_integrate(vol, cfg, d[f], e[f], None if images is None else images[f])
        got = want if images is not None else TC.ref_integrated(cfg, d, e)[0]
        assert vol.tobytes() == got.tobytes()
    assert (want["weight"] > 0).sum() > 100 and want["weight"].max() == 3 and (want["reserved"] == 0).all()
    assert np.isfinite(want["tsdf"]).all() and np.abs(want["tsdf"]).max() <= 1.0 + 1e-6


def test_ref_known_answer_plane():
    """A fronto-parallel plane at depth 2.0 under the identity pose. The voxel centres on both sides lie at 1.95 and 2.05:
    tsdf = +-0.05 / 0.3, alpha = 0.5, z = 1.95 + 0.05. The chain is fewer than ten fp32 operations near 2.0 (ulp 2.4e-7). The
    view covers 26 x 20 voxel columns: 520 points, all on the +z axis."""
    cfg = TC.scene_config(min_weight=1)
    vol = R.new_volume(cfg)
    assert R.integrate(vol, cfg, np.full((TC.H, TC.W), 2.0, f32), TC.pose())
    pts, total = R.extract(vol, cfg)
    err = np.abs(pts["X"][:, 2].astype(np.float64) - 2.0).max()
    print("points %d, max |z - 2| = %.3g" % (total, err))
    assert total == len(pts) >= 400
    assert err <= 1e-5
    assert (pts["axis"] == 2).all() and (pts["weight"] == 1).all()
    # behind the surface by more than trunc nothing is written; in front the value saturates at 1
    col = vol[:, 12, 16]
    assert (col["weight"][:11] == 1).all() and (col["weight"][11:] == 0).all() and (col["tsdf"][:4] == 1.0).all()


def test_ref_accuracy_on_the_analytic_scene():
    """Three poses (yaw 0, +0.15, -0.2 rad; x offset 0, -0.3, +0.35) of a plane at 2.4 and a sphere of radius 0.45; the metric
    is the distance of each point to the nearer surface. Measured with this restatement at voxel 0.1: 864 points, median
    0.00066, 95th percentile 0.0199 (the sphere's silhouette, where depth jumps inside one truncation band), maximum 0.062.
    Asserted: twice the measured values, which stay below voxel / 4 and voxel / 2."""
    cfg, vol, pts = TC.ref_scene()
    d = TC.surface_distance(pts["X"])
    med, p95 = np.median(d), np.percentile(d, 95)
    print("points %d, median %.5f, p95 %.5f, max %.5f" % (len(pts), med, p95, d.max()))
    bound_med, bound_p95 = 2 * 0.00066, 2 * 0.0199
    assert bound_med < TC.VOXEL / 4 and bound_p95 < TC.VOXEL / 2
    assert len(pts) >= 400 and med <= bound_med and p95 <= bound_p95


def test_ref_weight_cap_and_gray_rounding():
    """One voxel followed through five frames of the same view. max_weight = 2: w runs 1, 2, 2, 2, 2, so from the third frame on
    the running mean weighs the past with 2: tsdf and gray by hand."""
    cfg = TC.scene_config(max_weight=2, min_weight=1)
    depth = np.full((TC.H, TC.W), 2.0, f32)
    vol = R.new_volume(cfg)
    grays = (10, 13, 200, 0, 255)
    k, j, i = 7, 12, 16                                              # centre (0.05, 0.05, 1.95): sdf = 0.05, in view
    t, w, g = f32(0), 0, 0
    for n, gv in enumerate(grays):
        dn = depth + f32(0.01 * n)
        R.integrate(vol, cfg, dn, TC.pose(), np.full((TC.H, TC.W), gv, np.uint8))
        s = min(f32(1), (dn[0, 0] - f32(1.95)) * (f32(1) / cfg.trunc))
        t = (t * f32(w) + s) / (f32(w) + f32(1))
        g = (g * w + gv + ((w + 1) >> 1)) // (w + 1)
        w = min(w + 1, 2)
        rec = vol[k, j, i]
        assert (rec["tsdf"], int(rec["weight"]), int(rec["gray"])) == (t, w, g), n
    # the rounding rule itself: halves round up, the divisor is W0 + 1
    assert (0 * 0 + 7 + 0) // 1 == 7 and (7 * 1 + 8 + 1) // 2 == 8 and (8 * 2 + 9 + 1) // 3 == 8 and (3 * 2 + 5 + 1) // 3 == 4
    # without an image gray is untouched
    before = vol["gray"].copy()
    R.integrate(vol, cfg, depth, TC.pose())
    assert (vol["gray"] == before).all() and vol["weight"].max() == 2


def _loop_extract(vol, cfg):
    """Rule 4 voxel by voxel."""
    nx, ny, nz = cfg.dims
    out = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                a = vol[k, j, i]
                for axis, (kk, jj, ii) in enumerate(((k, j, i + 1), (k, j + 1, i), (k + 1, j, i))):
                    if ii >= nx or jj >= ny or kk >= nz:
                        continue
                    b = vol[kk, jj, ii]
                    if a["weight"] < cfg.min_weight or b["weight"] < cfg.min_weight or (a["tsdf"] < 0) == (b["tsdf"] < 0):
                        continue
                    alpha = a["tsdf"] / (a["tsdf"] - b["tsdf"])
                    p = np.zeros((), R.POINT_DTYPE)
                    X = [cfg.origin[n] + (f32(v) + f32(0.5)) * cfg.voxel for n, v in enumerate((i, j, k))]
                    X[axis] = X[axis] + alpha * cfg.voxel
                    p["X"], p["axis"] = X, axis
                    p["gray"] = a["gray"] if alpha < f32(0.5) else b["gray"]
                    p["weight"] = min(a["weight"], b["weight"])
                    out.append(p)
    return np.array(out, R.POINT_DTYPE)


def test_ref_extraction_equals_a_plain_per_voxel_loop():
    cfg, vol, pts = TC.ref_small()
    assert len(pts) > 100 and pts.tobytes() == _loop_extract(vol, cfg).tobytes()
    assert set(pts["axis"]) == {0, 1, 2}


def test_ref_zero_counts_as_non_negative_and_capacity_cut():
    cfg = R.config(dims=(8, 8, 8), voxel=1.0, origin=(0, 0, 0), min_weight=2)
    vol = R.new_volume(cfg)
    vol["weight"] = 2
    vol["tsdf"] = 0.5
    vol["tsdf"][0, 0, 0] = 0.0                                       # zero beside positive: no crossing
    vol["tsdf"][0, 0, 1] = -0.0                                      # minus zero is not < 0 either
    assert R.extract(vol, cfg)[1] == 0
    vol["tsdf"][2, 2, 2] = -0.5                                      # one negative voxel: six crossings around it
    vol["tsdf"][2, 2, 3] = 0.0                                       # its +x neighbour is zero: still a crossing, alpha = 1
    vol["tsdf"][2, 3, 2] = 1.0                                       # its +y neighbour: alpha = -0.5 / -1.5 = 1/3
    vol["gray"][2, 2, 2], vol["gray"][2, 2, 3], vol["gray"][2, 3, 2] = 11, 99, 55
    pts, total = R.extract(vol, cfg)
    assert total == 6
    assert pts.tobytes() == _loop_extract(vol, cfg).tobytes()        # canonical order: voxel a ascending, then the axis
    assert [(tuple(p["X"]), int(p["axis"])) for p in pts[3:]] == [
        ((3.5, 2.5, 2.5), 0), ((2.5, f32(2.5) + f32(-0.5) / f32(-1.5) * f32(1.0), 2.5), 1), ((2.5, 2.5, 3.0), 2)]
    px = pts[3]                                                      # a = (2, 2, 2) towards its zero neighbour:
    assert px["X"][0] == f32(2.5) + f32(1.0) and px["gray"] == 99 and px["weight"] == 2     # alpha = -0.5 / (-0.5 - 0) = 1
    assert pts[0]["gray"] == 11 and pts[5]["gray"] == 0 and pts[4]["gray"] == 11   # alpha = 0.5 takes b's gray, alpha = 1/3 a's
    # weights: one voxel below min_weight removes its crossings
    vol["weight"][2, 2, 1] = 1
    assert R.extract(vol, cfg)[1] == 5 and R.extract(vol, cfg, min_weight=1)[1] == 6 and R.extract(vol, cfg, min_weight=3)[1] == 0
    # the capacity cut: the first cap points, the full count
    vol["weight"][2, 2, 1] = 2
    for cap in (0, 1, 4, 6, 9):
        cut, tot = R.extract(vol, cfg, cap=cap)
        assert tot == 6 and cut.tobytes() == pts[:min(cap, 6)].tobytes()


def test_ref_skips_masked_and_non_finite_frames():
    cfg, want, _ = TC.ref_small()
    d, im, e = TC.small_frames()
    bad = e.copy()
    bad[1, 7] = np.nan
    vol, invalid = TC.ref_integrated(cfg, d, bad, im)
    only, _ = TC.ref_integrated(cfg, d[[0, 2]], e[[0, 2]], im[[0, 2]])
    assert invalid and vol.tobytes() == only.tobytes() and vol.tobytes() != want.tobytes()
    masked, invalid = TC.ref_integrated(cfg, d, bad, im, mask=[1, 0, 1])
    assert not invalid and masked.tobytes() == only.tobytes()


def test_tsdf_kernels_cross_compile_without_scratch():
    """From the compiler's resource metadata of the gfx950 listing: no private scratch in any kernel of the file, no LDS and
    no barrier in k_tsdf_integrate, no float atomics anywhere, and the correctly rounded divisions of rules 3c and 3g."""
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "tsdf_volume.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "tsdf_volume.hip")])
    text = open(path).read()
    for k in KERNELS:
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        hist, _, _ = S.stats(body)
        assert not any(op.startswith("global_atomic") and ("f32" in op or "f64" in op) for op in hist), k
    body, meta = S.kernel_body(text, "k_tsdf_integrate")
    hist, _, _ = S.stats(body)
    assert meta.get("LDSByteSize", -1) == 0 and "s_barrier" not in hist
    assert not any(op.startswith(("ds_", "global_atomic", "buffer_atomic")) for op in hist)
    assert hist["v_div_fixup_f32"] == 2                              # 1 / zc and the running mean
    assert not any(op.startswith(("v_fma_mix", "v_mad_f32", "v_mac_f32")) for op in hist)
    assert hist["global_load_dwordx2"] >= 1 and hist["global_store_dwordx2"] == 1          # the record: one load, one store
    assert sum(n for op, n in hist.items() if op.startswith("s_load_dword")) >= 3         # frame records through scalar loads


def test_tsdf_volume_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "tsdf_volume.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "tsdf_volume.hip")).read()
    assert "std::getenv" not in src and "asm" not in src.replace("aria_slam_amd", "")
    assert math.isclose(R.DEFAULTS["voxel"], 0.05)
