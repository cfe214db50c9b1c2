"""Two-view triangulation and point map (include/aria_orb_hip.h, "two-view triangulation and point map"): the parts that need
no GPU -- exports, record layouts and defaults, the NumPy restatement (aria_slam_amd/map_ref.py) on known answers, filter
semantics, the export formats, the triangulation kernel's listing and the C++ adapter build."""
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
import map_cases   # noqa: E402

MAP_SYMBOLS = ["aria_map_default_config", "aria_map_create", "aria_map_destroy", "aria_map_stream", "aria_map_check",
               "aria_map_triangulate", "aria_map_triangulate_batch_device", "aria_map_points_needed", "aria_map_size",
               "aria_map_capacity", "aria_map_clear", "aria_map_reserve", "aria_map_read", "aria_map_device_points",
               "aria_map_filter_outliers", "aria_map_filter_distance"]

# a scene whose projections are exact in fp32: K and depths are powers of two, coordinates multiples of 1/64
DYADIC_K = (512.0, 512.0, 320.0, 240.0)


def test_map_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in MAP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipMapper" in aria.__all__


def test_map_record_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    dt = _lib.MAP_POINT_DTYPE
    assert dt.itemsize == 72
    assert [dt.fields[k][1] for k in ("id", "X", "quality", "err", "pair", "match", "idx1", "idx2", "gray")] == \
        [0, 8, 32, 40, 48, 52, 56, 60, 64]
    assert C.sizeof(_lib.MapConfig) == 96
    cfg = _lib.MapConfig()
    aria.load_library().aria_map_default_config(C.byref(cfg))
    assert cfg.struct_size == 96
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375)
    assert (cfg.min_depth, cfg.max_depth, cfg.min_parallax_deg, cfg.max_reproj_px) == (0.1, 50.0, 1.0, 2.0)
    assert cfg.capacity == 65536 and cfg.min_pose_inliers == 10 and not cfg.stream


def _dyadic_scene(n=64, seed=0):
    from aria_slam_amd import map_ref as M
    rng = np.random.default_rng(seed)
    X = np.stack([rng.integers(-64, 64, n) / 64, rng.integers(-48, 48, n) / 64, 2.0 ** rng.integers(1, 4, n)], 1)
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    E1, E2 = M.extrinsics(np.eye(3), [0, 0, 0]), M.extrinsics(Rz, [-1, 0.5, 0])
    return X, E1, E2


def _project(E, X, K):
    c = X @ E[:, :3].T + E[:, 3]
    return np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], 1)


def test_map_ref_recovers_a_noise_free_scene():
    from aria_slam_amd import map_ref as M
    X, E1, E2 = _dyadic_scene()
    x1, x2 = _project(E1, X, DYADIC_K), _project(E2, X, DYADIC_K)
    assert np.array_equal(x1, x1.astype(np.float32)) and np.array_equal(x2, x2.astype(np.float32))
    reason, Xr, err = M.triangulate_points(x1, x2, E1, E2, DYADIC_K)
    assert (reason == M.KEPT).all()
    assert (np.linalg.norm(Xr - X, axis=1) / np.linalg.norm(X, axis=1)).max() < 1e-9
    assert err.max() < 1e-6
    # a general scene (rotations, EuRoC K): fp32 pixel rounding bounds the error, not the solver
    E1 = M.extrinsics(M.rot([0, 1, 0.2], 10), [0.3, -0.1, 0.5])
    E2 = M.extrinsics(M.rot([0.1, 1, 0], -5) @ M.rot([0, 1, 0.2], 10), [1.2, 0.1, 0.4])
    kq, kt, m, Xw, _ = M.synth_scene(1, 500, E1, E2, noise_px=0.0)
    pts = M.triangulate_pair(kq, kt, m, E1, E2)
    assert len(pts) == 500 and np.array_equal(pts["match"], np.arange(500))
    assert (np.linalg.norm(pts["X"] - Xw, axis=1) / np.linalg.norm(Xw, axis=1)).max() < 1e-5


def test_map_ref_each_rejection_rule_fires():
    from aria_slam_amd import map_ref as M
    K = DYADIC_K
    E1, E2 = M.extrinsics(np.eye(3), [0, 0, 0]), M.extrinsics(np.eye(3), [-1, 0, 0])

    def one(X, dx2=0.0):
        X = np.asarray(X, np.float64).reshape(1, 3)
        x1, x2 = _project(E1, X, K), _project(E2, X, K)
        x2[0, 1] += dx2                                          # across the epipolar line (horizontal)
        return M.triangulate_points(x1, x2, E1, E2, K)[0][0]

    assert one([0.25, 0.125, 4.0]) == M.KEPT
    # behind both cameras: the projections are those of the mirrored point; the DLT returns the point behind
    assert one([0.25, 0.125, -4.0]) == M.DEPTH
    assert one([0.25, 0.125, 64.0]) == M.DEPTH                    # beyond max_depth (50)
    b = 0.25 / np.tan(np.deg2rad(0.5))                            # ~0.5 degree parallax at depth b (28.6): depth passes
    E2p = M.extrinsics(np.eye(3), [-0.25, 0, 0])
    X = np.array([[0.125, 0.0, b]])
    r = M.triangulate_points(_project(E1, X, K), _project(E2p, X, K), E1, E2p, K)[0][0]
    assert r == M.PARALLAX
    assert one([0.25, 0.125, 4.0], dx2=6.0) == M.REPROJ           # 6 px off the epipolar line: ~3 px per view
    # a point at infinity: identical pixels under a pure translation -> X[3] = 0
    x = np.array([[320.0, 240.0]])
    assert M.triangulate_points(x, x, E1, E2, K)[0][0] == M.AT_INFINITY


def test_map_ref_pair_gate_mask_gray_and_order():
    from aria_slam_amd import map_ref as M
    E1 = M.extrinsics(np.eye(3), [0, 0, 0])
    E2 = M.extrinsics(M.rot([0, 1, 0], -5), [-1.0, 0, 0.2])
    kq, kt, m, Xw, _ = M.synth_scene(4, 40, E1, E2, noise_px=0.0)
    assert len(M.triangulate_pair(kq, kt, m[:7], E1, E2)) == 0      # Mapper.cpp:13: fewer than 8 matches
    assert len(M.triangulate_pair(kq, kt, m[:8], E1, E2)) == 8
    mask = np.zeros(40, np.uint8)
    mask[::3] = 1
    pts = M.triangulate_pair(kq, kt, m, E1, E2, mask=mask, pair=7)
    assert np.array_equal(pts["match"], np.arange(0, 40, 3)) and (pts["pair"] == 7).all() and (pts["gray"] == 127).all()
    img = (np.arange(480 * 752) % 251).astype(np.uint8).reshape(480, 752)
    pts = M.triangulate_pair(kq, kt, m, E1, E2, image=img)
    xs = np.clip(kq["x"].astype(np.int64), 0, 751)
    ys = np.clip(kq["y"].astype(np.int64), 0, 479)
    assert np.array_equal(pts["gray"], img[ys, xs])
    assert np.allclose(pts["quality"], 1.0 / (pts["err"][:, 0].astype(np.float64) + pts["err"][:, 1] + 0.1), rtol=1e-6)
    # swapped roles: view 1 is the train side
    sw = m.copy()
    sw["query_idx"], sw["train_idx"] = m["train_idx"], m["query_idx"]
    pts2 = M.triangulate_pair(kt, kq, sw, E1, E2, query_is_first=False)
    assert np.array_equal(pts2["X"], M.triangulate_pair(kq, kt, m, E1, E2)["X"])


def test_map_ref_default_dtype_is_float64_bit_for_bit():
    """The dtype argument of the restatement: the default call and the explicit np.float64 call give the same bytes, and an
    np.longdouble run returns that type."""
    from aria_slam_amd import map_ref as M
    kq, kt, m, E1, E2 = map_cases.ref_scene(1)
    x1, x2 = map_cases.pixels(kq, kt, m)
    for a, b in zip(M.triangulate_points(x1, x2, E1, E2), M.triangulate_points(x1, x2, E1, E2, dtype=np.float64)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    A = np.random.default_rng(2).normal(size=(50, 4, 4))
    assert M.dlt_null_vectors(A).tobytes() == M.dlt_null_vectors(A, dtype=np.float64).tobytes()
    assert M.projection(M.EUROC_K, E2).tobytes() == M.projection(M.EUROC_K, E2, dtype=np.float64).tobytes()
    assert M.as_extrinsics(np.eye(4)).tobytes() == M.as_extrinsics(np.eye(4), dtype=np.float64).tobytes()
    reason, X, err = M.triangulate_points(x1, x2, E1, E2, dtype=np.longdouble)
    assert X.dtype == err.dtype == np.longdouble and M.projection(M.EUROC_K, E2, np.longdouble).dtype == np.longdouble
    assert np.array_equal(reason, M.triangulate_points(x1, x2, E1, E2)[0])


@pytest.mark.parametrize("name", map_cases.SCENES)
def test_map_ref_committed_scenes_stay_clear_of_the_thresholds(name):
    """The device tests compare the kept set with the extended run of the restatement without a margin. That is sound because
    no tested quantity of that run lies within 1e-9 (relative) of its threshold on the committed seeds, about five decades
    above what separates two correct evaluations (tools/map_gap.py). A seed that fails here is to be changed."""
    f64, ext = map_cases.ref_runs(name)
    assert ext["margin"].min() >= 1e-9, (name, float(ext["margin"].min()))
    assert np.array_equal(f64["keep"], ext["keep"]) and ext["keep"].sum() >= 100


def test_map_ref_rejects_non_finite_keypoints():
    """NaN, +Inf, -Inf and 3e38 in a keypoint coordinate of either view: the match is rejected, the others are untouched."""
    from aria_slam_amd import map_ref as M
    kq, kt, m, E1, E2, bad = map_cases.nonfinite_pair()
    assert len(bad) == 12 and len(set(bad // 64)) == 3
    x1, x2 = map_cases.pixels(kq, kt, m)
    assert sorted(np.flatnonzero(~(np.isfinite(x1).all(1) & np.isfinite(x2).all(1) & (np.abs(x1).max(1) < 1e38) &
                                   (np.abs(x2).max(1) < 1e38)))) == sorted(bad)
    with np.errstate(all="ignore"):
        reason, X, err = M.triangulate_points(x1, x2, E1, E2)
    assert (reason[bad] != M.KEPT).all(), reason[bad]
    ok = np.setdiff1d(np.arange(600), bad)
    clean = M.triangulate_points(x1[ok], x2[ok], E1, E2)
    assert np.array_equal(reason[ok], clean[0]) and (clean[0] == M.KEPT).sum() > 400
    assert X[ok].tobytes() == clean[1].tobytes() and err[ok].tobytes() == clean[2].tobytes()
    mask = np.ones(600, np.uint8)
    mask[bad] = 0
    with np.errstate(all="ignore"):
        assert M.triangulate_pair(kq, kt, m, E1, E2).tobytes() == M.triangulate_pair(kq, kt, m, E1, E2, mask=mask).tobytes()


def _planted(n, far, seed=0):
    from aria_slam_amd._lib import MAP_POINT_DTYPE
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, MAP_POINT_DTYPE)
    pts["X"] = rng.normal(0, 1.0, (n, 3))
    pts["X"][far] = [[40.0 * (k + 1), 0, 0] for k in range(len(far))]
    pts["id"] = np.arange(100, 100 + n)
    return pts


def test_map_ref_filters():
    from aria_slam_amd import map_ref as M
    pts = _planted(9, [3])
    assert np.array_equal(M.filter_outliers(pts), pts)                # no-op below 10 points
    pts = _planted(200, [5, 77, 150])
    kept = M.filter_outliers(pts)
    assert len(kept) == 197 and np.array_equal(kept["id"], np.delete(pts["id"], [5, 77, 150]))
    d = M.filter_distance(pts, 2.0)
    r = np.linalg.norm(pts["X"], axis=1)
    assert np.array_equal(d["id"], pts["id"][r <= 2.0])
    m = M.Map()
    m.append(pts[:3])
    m.append(pts[3:5])
    assert list(m.points["id"]) == [0, 1, 2, 3, 4] and m.next_id == 5
    m.filter_distance(0.0)
    m.append(pts[:1])
    assert list(m.points["id"]) == [5]


def test_export_headers_are_the_references():
    from aria_slam_amd import mapper
    from aria_slam_amd._lib import MAP_POINT_DTYPE
    # Mapper::exportPLY / exportPCD (src/legacy/Mapper.cpp:170-235), verbatim
    ply = ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    pcd = ("# .PCD v0.7 - Point Cloud Data\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
           "WIDTH 2\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 2\nDATA ascii\n")
    pts = np.zeros(2, MAP_POINT_DTYPE)
    pts["X"] = [[1.0, -0.5, 12.3456789], [1e-5, 123456789.0, -0.0]]
    pts["gray"] = [127, 3]
    assert mapper.ply_text(pts) == ply + "1 -0.5 12.3457 127 127 127\n1e-05 1.23457e+08 -0 3 3 3\n"
    assert mapper.pcd_text(pts) == pcd + "1 -0.5 12.3457 %d\n1e-05 1.23457e+08 -0 %d\n" % (127 * 65793, 3 * 65793)


def test_triangulation_kernel_cross_compiles_without_scratch():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "map_triangulate.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "map_triangulate.hip")])
    text = open(path).read()
    for k in ("k_map_tri", "k_map_scan", "k_map_scatter", "k_map_psum", "k_map_stats", "k_map_flag", "k_map_fscan",
              "k_map_fscatter"):
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
    in_loop, outside = S.scratch_accesses(text, "k_map_tri")
    assert not in_loop and not outside


def test_map_triangulate_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "map_triangulate.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "map_triangulate.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in src)
    assert "getenv" not in src



def test_host_adapters_build_with_the_mapper(aria):
    pkg = os.path.join(ROOT, "aria_slam_amd")
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host"), "-s"])
    syms = subprocess.run(["nm", "-DC", os.path.join(pkg, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipMapper::triangulate", "aria::adapters::hip::HipMapper::exportPLY",
                 "aria::adapters::hip::HipMapper::filterOutliers", "aria::adapters::hip::HipMapper::triangulateExtrinsics"):
        assert name in syms, name
    usage = subprocess.run([os.path.join(pkg, "euroc_frontend")], capture_output=True, text=True)
    assert "--map" in usage.stderr
