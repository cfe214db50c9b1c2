"""Rectification (include/aria_orb_hip.h, "rectification"): the parts that need no GPU -- exports, structure layouts, defaults
and config validation, the host-only stereo geometry against the NumPy restatement (aria_slam_amd/rectify_ref.py, which is
the definition) bit for bit, the geometric properties of that restatement on the EuRoC MH calibration, the map and point
steps on known answers, the sensor.yaml reader, and the accuracy of the definition on a synthetic raw stereo pair."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as RC   # noqa: E402

RECT_SYMBOLS = ["aria_rect_default_config", "aria_rect_create", "aria_rect_destroy", "aria_rect_stream", "aria_rect_check",
                "aria_rect_stereo_geometry", "aria_rect_remap_batch_device", "aria_rect_remap", "aria_rect_points_batch_device",
                "aria_rect_points", "aria_rect_get_map", "aria_rect_algorithmic_bytes"]


def test_rect_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in RECT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipRectifier" in aria.__all__ and "load_sensor_yaml" in aria.__all__
    assert L.aria_rect_algorithmic_bytes(752, 480) == 2 * 752 * 480


def test_rect_layouts_and_defaults(aria):
    from aria_slam_amd import _lib, rectify_ref
    assert C.sizeof(_lib.RectCamera) == 144 and C.sizeof(_lib.RectConfig) == 368
    cfg = _lib.RectConfig()
    aria.load_library().aria_rect_default_config(C.byref(cfg))
    assert cfg.struct_size == 368 and not cfg.stream and cfg.n_cameras == 1 and cfg.fill == 0
    assert (cfg.src_width, cfg.src_height, cfg.dst_width, cfg.dst_height) == (752, 480, 752, 480)
    c = cfg.cam[0]
    assert (c.fx, c.fy, c.cx, c.cy) == rectify_ref.EUROC_K == RC.K_L                 # EuRoC cam0
    assert tuple(c.dist) == rectify_ref.EUROC_D == RC.D_L + (0.0,)
    assert tuple(c.R) == rectify_ref.IDENTITY                                        # plain undistortion
    assert (cfg.new_fx, cfg.new_fy, cfg.new_cx, cfg.new_cy) == rectify_ref.EUROC_K   # new K = K
    m = rectify_ref.EUROC_MH                                                         # the rig of the tools = the one typed here
    assert (m["K_l"], m["K_r"], m["D_l"], m["D_r"], m["size"]) == (RC.K_L, RC.K_R, RC.D_L, RC.D_R, RC.SIZE)
    assert list(m["T_BS_l"]) == RC.T_BS_L and list(m["T_BS_r"]) == RC.T_BS_R


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("struct_size", 360), ("src_width", 1), ("src_height", 2048),
                                         ("dst_width", 0), ("dst_height", 2048), ("n_cameras", 0), ("n_cameras", 3),
                                         ("new_fx", 0.0), ("new_fy", -1.0), ("new_cx", float("nan")), ("fill", 256)])
def test_rect_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.RectConfig()
    L.aria_rect_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1       # ARIA_E_INVALID
    assert not h.value
    assert L.aria_rect_create(None, C.byref(h)) == -1
    assert L.aria_rect_check(None) == -1


def test_rect_calls_refuse_null_handles(aria):
    L = aria.load_library()
    assert L.aria_rect_remap_batch_device(None, 0, None, 0, 752, 1, None, 0, 752) == -1
    assert L.aria_rect_points_batch_device(None, 0, None, None, 1, 1, None) == -1
    assert L.aria_rect_get_map(None, 0, None, 0) == -1 and L.aria_rect_stream(None) is None


@pytest.mark.parametrize("field,value", [("fx", 0.0), ("fy", -3.0), ("fx", float("inf")), ("cx", float("nan"))])
def test_rect_camera_validation(aria, field, value):
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.RectConfig()
    L.aria_rect_default_config(C.byref(cfg))
    setattr(cfg.cam[0], field, value)
    h = C.c_void_p()
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1 and not h.value


def _c_geometry(aria, new_K=None):
    from aria_slam_amd import _lib
    cfg = _lib.RectConfig()
    if new_K is not None:
        cfg.new_fx, cfg.new_fy, cfg.new_cx, cfg.new_cy = new_K
    a = [np.asarray(v, np.float64) for v in (RC.K_L, RC.K_R, RC.T_BS_L, RC.T_BS_R)]
    b = C.c_double(0.0)
    rc = aria.load_library().aria_rect_stereo_geometry(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                                       C.byref(cfg), C.byref(b))
    assert rc == 0
    return cfg, b.value


def test_stereo_geometry_equals_the_restatement_bitwise(aria):
    from aria_slam_amd import rectify_ref as R
    for new_K in (None, RC.SMALL_NEW_K, (0.0, 300.0, 0.0, 200.0)):
        cfg, baseline = _c_geometry(aria, new_K)
        g = R.stereo_geometry(RC.K_L, RC.K_R, RC.T_BS_L, RC.T_BS_R, new_K)
        assert np.array(cfg.cam[0].R[:]).tobytes() == g["R1"].tobytes()
        assert np.array(cfg.cam[1].R[:]).tobytes() == g["R2"].tobytes()
        assert (cfg.new_fx, cfg.new_fy, cfg.new_cx, cfg.new_cy) == g["new_K"]
        assert np.float64(baseline).tobytes() == np.float64(g["baseline"]).tobytes()
    g = R.stereo_geometry(RC.K_L, RC.K_R, RC.T_BS_L, RC.T_BS_R, (0.0, 300.0, 0.0, 200.0))
    f = (RC.K_L[1] + RC.K_R[1]) / 2
    assert g["new_K"] == (f, 300.0, (RC.K_L[2] + RC.K_R[2]) / 2, 200.0)           # only the zeros take the default
    assert aria.load_library().aria_rect_stereo_geometry(None, None, None, None, None, None) == -1


def test_stereo_geometry_properties():
    """On the EuRoC MH calibration: R1, R2 orthonormal, R2 R R1^T = I, projected 3-D points on one row, positive
    disparities, the rig's 11 cm baseline."""
    from aria_slam_amd import rectify_ref as R
    g = R.stereo_geometry(RC.K_L, RC.K_R, RC.T_BS_L, RC.T_BS_R)
    R1, R2, Rm, t = g["R1"], g["R2"], g["R"], g["t"]
    eye = np.eye(3)
    assert np.abs(R1 @ R1.T - eye).max() <= 1e-14 and np.abs(R2 @ R2.T - eye).max() <= 1e-14
    assert np.abs(R2 @ Rm @ R1.T - eye).max() <= 1e-14
    assert abs(np.linalg.det(R1) - 1) <= 1e-14 and abs(np.linalg.det(R2) - 1) <= 1e-14
    assert abs(g["baseline"] - 0.1101) <= 1e-4
    fx, fy, cx, cy = g["new_K"]
    rng = np.random.default_rng(5)
    X = np.stack([rng.uniform(-3, 3, 500), rng.uniform(-2, 2, 500), rng.uniform(0.5, 20, 500)], axis=1)   # left camera frame
    pl = X @ R1.T
    pr = (X @ Rm.T + t) @ R2.T
    ul, vl = fx * pl[:, 0] / pl[:, 2] + cx, fy * pl[:, 1] / pl[:, 2] + cy
    ur, vr = fx * pr[:, 0] / pr[:, 2] + cx, fy * pr[:, 1] / pr[:, 2] + cy
    print("row difference %.3g px, least disparity %.3g px, baseline %.6f m" % (np.abs(vl - vr).max(), (ul - ur).min(), g["baseline"]))
    assert np.abs(vl - vr).max() <= 1e-9
    assert (ul - ur).min() > 0
    assert np.abs((ul - ur) - fx * g["baseline"] / pl[:, 2]).max() <= 1e-9          # disparity = f b / depth


def test_points_invert_the_distortion():
    """undistort_points(distort(p)) = p within 1e-6 px over a grid that covers the raw image, plain and rectified."""
    from aria_slam_amd import rectify_ref as R
    cam0 = R.camera(RC.K_L, RC.D_L)
    ys, xs = np.mgrid[0:480:8, 0:752:8].astype(np.float64)
    grid = np.stack([xs.ravel(), ys.ravel()], axis=1)
    ideal = R.undistort_points(grid, cam0, RC.K_L)                  # where the raw grid lies in the ideal image
    for p in (grid, ideal):
        raw = R.distort(p, cam0)
        back = R.undistort_points(raw, cam0, RC.K_L)
        err = np.abs(back - p).max()
        print("round trip over %d points: %.3g px" % (len(p), err))
        assert back.dtype == np.float64 and err <= 1e-6
    assert np.abs(R.distort(ideal, cam0) - grid).max() <= 1e-6      # and the other way round: the raw corners come back
    # records: fp32 in and out, every other field kept, the rotation applied
    cl, cr, nk, _ = RC.cameras(None)
    kp, counts = RC.keypoints()
    out = R.undistort_points(kp[2], cr, nk)
    assert out.dtype == kp.dtype and all(np.array_equal(out[f], kp[2][f]) for f in ("size", "angle", "response", "octave"))
    u, v, Z = R.undistort_xy(kp[2]["x"], kp[2]["y"], cr, nk)
    assert np.array_equal(out["x"], u.astype(np.float32)) and np.array_equal(out["y"], v.astype(np.float32)) and (Z > 0).all()


def test_points_never_write_nan_or_inf():
    from aria_slam_amd import rectify_ref as R
    from aria_slam_amd._lib import KP_DTYPE
    cam = R.camera(RC.K_L, (5.0, 40.0, 0.1, 0.1, 300.0), [0, 0, 1, 0, 1, 0, -1, 0, 0])   # wild distortion, a quarter turn
    k = np.zeros(6, KP_DTYPE)
    k["x"] = [0, 751, 3e38, -3e38, 367.215, 1e20]
    k["y"] = [0, 479, 3e38, 3e38, 248.375, -1e20]
    out = R.undistort_points(k, cam, RC.K_L)
    assert np.isfinite(out["x"]).all() and np.isfinite(out["y"]).all()
    assert ((out["x"] == -1) & (out["y"] == -1)).any()


def test_identity_calibration_returns_the_image():
    """D = 0, R = I, new K = K: the image comes back unchanged on all but the last row and column, which the invalid rule
    (ix + 1 > W - 1) fills."""
    from aria_slam_amd import rectify_ref as R
    W, H = 97, 61
    cam = R.camera((80.5, 79.25, 47.3, 30.9))
    m = R.build_map(cam, cam["K"], W, H, W, H)
    ok = m != R.INVALID
    assert ok[:-1, :-1].all() and not ok[-1, :].any() and not ok[:, -1].any()
    ys, xs = np.mgrid[0:H - 1, 0:W - 1]
    assert np.array_equal(m[:-1, :-1], (xs * 32 | (ys * 32) << 16).astype(np.uint32))
    img = np.random.default_rng(6).integers(0, 256, (H, W), dtype=np.uint8)
    out = R.remap(img, m, fill=9)
    assert np.array_equal(out[:-1, :-1], img[:-1, :-1]) and (out[-1, :] == 9).all() and (out[:, -1] == 9).all()


def test_map_known_answers():
    """A pure shift by (2.5, 1.25) px through new cx', cy' gives a constant fraction (16, 8) and the bilinear mean; a
    destination that looks behind the camera (Z <= 0) is invalid."""
    from aria_slam_amd import rectify_ref as R
    W, H = 40, 30
    cam = R.camera((50.0, 50.0, 20.0, 15.0))
    m = R.build_map(cam, (50.0, 50.0, 17.5, 13.75), W, H, W, H)
    ok = m != R.INVALID
    assert ((m[ok] & 31) == 16).all() and (((m[ok] >> 16) & 31) == 8).all()
    assert m[0, 0] == (2 * 32 + 16) | ((1 * 32 + 8) << 16)
    img = np.random.default_rng(7).integers(0, 256, (H, W), dtype=np.uint8).astype(np.int64)
    out = R.remap(img.astype(np.uint8), m)
    want = (img[1, 2] * 16 * 24 + img[1, 3] * 16 * 24 + img[2, 2] * 16 * 8 + img[2, 3] * 16 * 8 + 512) >> 10
    assert out[0, 0] == want
    behind = R.camera((50.0, 50.0, 20.0, 15.0), R=[1, 0, 0, 0, -1, 0, 0, 0, -1])   # half a turn about x
    assert (R.build_map(behind, (50.0, 50.0, 20.0, 15.0), W, H, W, H) == R.INVALID).all()


def test_small_shape_is_a_real_test_of_the_map():
    """Shape (a2): between 10 % and 30 % invalid, every value of fx5 and fy5 present."""
    from aria_slam_amd import rectify_ref as R
    for m in RC.ref_maps(True):
        ok = m != R.INVALID
        assert 0.10 < 1 - ok.mean() < 0.30
        assert len(np.unique(m[ok] & 31)) == 32 and len(np.unique((m[ok] >> 16) & 31)) == 32


def test_read_forms_on_hand_made_lanes():
    """read_forms against lanes written by hand: the span bounds (x-span 6 and y-span 1 are the last of the rows form), the
    right-edge term, the padded tail lane, a lane without a valid pixel."""
    from aria_slam_amd import rectify_ref as R
    w = lambda ix, iy: np.uint32((ix << 5) | (iy << 21) | 9)   # noqa: E731
    X = np.uint32(R.INVALID)
    m = np.array([[w(10, 5), w(12, 5), w(14, 6), w(16, 5),   w(10, 5), w(12, 5), w(14, 5), w(17, 5),   w(3, 7), X],
                  [w(10, 5), w(10, 6), w(10, 7), w(10, 5),   X, X, X, X,                               w(25, 0), w(24, 1)],
                  [w(24, 9), X, w(30, 9), X,                 w(25, 9), w(31, 9), w(25, 9), w(25, 9),   X, X]], np.uint32)
    f = RC.read_forms(m, 32)
    assert f["form"].tolist() == [[RC.ROWS, RC.TAPS, RC.ROWS], [RC.TAPS, RC.NONE, RC.ROWS], [RC.ROWS, RC.TAPS, RC.NONE]]
    assert f["xspan"].tolist() == [[6, 7, 0], [0, -1, 1], [6, 6, -1]] and f["yspan"].tolist() == [[1, 0, 0], [2, -1, 1], [0, 0, -1]]
    assert f["edge_only"].tolist() == [[False, False, False], [False, False, False], [False, True, False]]
    assert f["mixed"].tolist() == [[False, False, True], [False, False, True], [True, False, False]]   # the padded tail counts
    assert f["x0"][0, 0] == 10 and f["y0"][0, 0] == 5 and f["x0"][1, 2] == 24 and f["y0"][1, 2] == 0
    assert RC.read_forms(m, 33)["form"][2, 1] == RC.ROWS                  # one more source column: x0 + 7 is inside


def test_edge_cases_reach_their_branches():
    """What each case of rectify_cases.EDGE_CASES is for, asserted on the restatement's map with slack, so that a change of
    the inputs cannot silently empty a branch. The figures seen are in DESIGN.md section 19."""
    from aria_slam_amd import rectify_ref as R
    n = {name: RC.form_counts(c) for name, c in RC.EDGE_CASES.items()}
    for name, c in n.items():
        print(name, c)
    c = n["zoom45"]                                                        # both sides of the x-span bound
    assert c["xspan6"] >= 20 and c["xspan7"] >= 10 and c["rows"] >= 100 and c["mixed"] >= 10 and c["edge_only"] >= 10
    c = n["zoom20"]
    assert c["xspan_max"] >= 12 and c["yspan2"] >= 1 and c["rows"] >= 20 and c["taps"] >= 20
    c = n["roll20"]                                                        # both sides of the y-span bound, the + 64 shift
    assert c["yspan1"] >= 100 and c["yspan2"] >= 50 and c["low_pair"] >= 100
    c = n["roll90"]
    assert c["rows"] == 0 and c["taps"] == c["lanes"] and c["yspan_max"] >= 2 and c["invalid_share"] < 0.02
    c = n["yaw75"]
    Z = R.source_coords(RC.EDGE_CASES["yaw75"].cam, RC.EDGE_CASES["yaw75"].new_K, 41, 33)[2]
    assert (Z <= 0).sum() >= 100 and c["rows"] >= 20 and c["taps"] >= 20
    c = n["src8"]
    assert c["taps"] >= 1 and c["rows"] == 0 and c["edge_only"] == c["taps"]
    c = n["src2"]
    assert (RC.EDGE_CASES["src2"].map != R.INVALID).sum() >= 1 and c["lanes"] == 1 and RC.EDGE_CASES["src2"].dst[0] < 4
    assert sum(n[k]["mixed_rows"] for k in RC.DEVICE_CASES) >= 50          # valid and invalid pixels in one rows-form lane
    # the lower-row clamp: a rows-form lane whose taps all lie in row src_h - 2, so that row y0 + 2 would be below the image
    assert n["zoom45"]["last_row"] + n["roll20"]["last_row"] >= 5 and n["limits"]["last_row"] >= 100
    # the limits of the 11 + 5 bit packing
    m = RC.EDGE_CASES["limits"].map
    ok = m != R.INVALID
    ix, iy = (m & 0xFFFF) >> 5, m >> 21
    assert RC.EDGE_CASES["limits"].src == (R.MAX_DIM, R.MAX_DIM) == (2047, 2047)
    assert (ix[ok] == 2045).any() and (iy[ok] == 2045).any() and ((m[ok] >> 31) == 1).any()
    assert ok[:23, :2046].all() and not ok[:, 2046].any() and not ok[23].any()   # one pixel further is invalid
    assert n["limits"]["rows"] >= 1000 and n["limits"]["edge_only"] >= 20
    # the variants' LDS form: tiles that are staged and tiles that are not
    box = RC.tile_box_bytes(RC.EDGE_CASES["zoom20_big"].map)
    assert (box > RC.LDS_BYTES).any() and ((box > 0) & (box <= RC.LDS_BYTES)).any()
    # the layouts: one tight case whose every row is stored by dwords, fill = 255 once, 17 frames = groups of 8, 8 and 1
    tight = [c for c in RC.EDGE_CASES.values() if c.dst_pitch == c.dst[0]]
    assert [c.name for c in tight] == ["roll90"] and tight[0].dst[0] % 4 == 0 and tight[0].src_pitch == tight[0].src[0]
    assert sorted(c.fill for c in RC.EDGE_CASES.values()).count(255) == 1
    assert all(c.dst_pitch % 2 == 1 and c.src_pitch > c.src[0] for c in RC.EDGE_CASES.values() if c not in tight)
    assert all(RC.EDGE_CASES[k].n_frames == 17 for k in RC.DEVICE_CASES if k != "limits")
    for c in RC.EDGE_CASES.values():                                       # noise: a wrong tap shows
        assert len(np.unique(c.frames)) == 256 or c.frames.size < 4096


def test_edge_points_reach_both_outcomes():
    """The points cases: the four non-finite records give (-1, -1) on the identity camera and nothing else does; each rotated
    camera has at least 50 records at (-1, -1) by Z <= 0 and at least 50 finite ones. Nothing written is NaN or infinite."""
    n = RC.POINT_COUNTS[0]
    for name, (want, behind) in RC.ref_edge_points_all().items():
        gone = (want[0, :n]["x"] == -1) & (want[0, :n]["y"] == -1)
        print(name, int(gone.sum()), "at (-1, -1),", int((gone & behind).sum()), "by Z <= 0")
        assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()
        assert gone[RC.POINT_NONFINITE].all() and (gone | ~behind).all()
        if name == "identity":
            assert np.nonzero(gone)[0].tolist() == RC.POINT_NONFINITE
        else:
            assert (gone & behind).sum() >= 50 and (~gone).sum() >= 50


def test_load_sensor_yaml(aria, tmp_path):
    p = str(tmp_path / "sensor.yaml")
    RC.write_sensor_yaml(p, RC.K_R, RC.D_R, RC.T_BS_R)
    s = aria.load_sensor_yaml(p)
    assert s["K"] == RC.K_R and s["dist"] == RC.D_R + (0.0,) and s["resolution"] == RC.SIZE
    assert np.array_equal(s["T_BS"], np.array(RC.T_BS_R).reshape(4, 4))
    one = str(tmp_path / "one_line.yaml")                           # data on one line, five coefficients, no resolution
    with open(one, "w") as f:
        f.write("T_BS:\n  cols: 4\n  rows: 4\n  data: [%s]\nintrinsics: [1.5, 2.5, 3.5, 4.5]\n"
                "distortion_coefficients: [0.1, 0.2, 0.3, 0.4, 0.5]\n" % ", ".join(repr(float(v)) for v in range(16)))
    s = aria.load_sensor_yaml(one)
    assert s["K"] == (1.5, 2.5, 3.5, 4.5) and s["dist"] == (0.1, 0.2, 0.3, 0.4, 0.5) and s["resolution"] is None
    assert np.array_equal(s["T_BS"], np.arange(16.0).reshape(4, 4))
    bad = str(tmp_path / "bad.yaml")
    with open(bad, "w") as f:
        f.write("rate_hz: 20\n")
    with pytest.raises(ValueError):
        aria.load_sensor_yaml(bad)
    with open(bad, "w") as f:
        f.write("intrinsics: [1, 2, 3, 4]\ndistortion_model: equidistant\ndistortion_coefficients: [0, 0, 0, 0]\n")
    with pytest.raises(ValueError):                                 # the fisheye model is out of scope
        aria.load_sensor_yaml(bad)


# ---- accuracy of the definition -----------------------------------------------------------------------------------------
# The margins come from what the two extra bilinear resamplings (rectified -> raw when the pair is made, raw -> rectified by
# the stage) can do, not from the figures below. Matched share: the resamplings blur, they do not move, so the share may
# drop only by what the border loses; 5 points. Median |disparity error|: a bilinear tap pair spreads a step edge over up to
# one more pixel, at a sampling phase that differs between the two views, and the stage's map rounds every coordinate to
# 1/32 px; the three-point parabola through a SAD curve whose two flanks are blurred by different amounts is off by up to a
# quarter of that pixel: 0.25 px over both resamplings.
SHARE_MARGIN, MEDIAN_MARGIN = 0.05, 0.25


@pytest.fixture(scope="module")
def accuracy(oracle):
    from aria_slam_amd import rectify_ref as R
    from aria_slam_amd import stereo_ref as S
    W, H = 320, 240
    cal = R.scaled_calibration(W, H, RC.EUROC)
    cl, cr, nk, _ = R.rectified_cameras(cal)
    maps = [R.build_map(c, nk, W, H, W, H) for c in (cl, cr)]
    p = oracle.default_params(500)

    def chain(left, right, d):
        kl, dl = oracle.orb_extract(left, p)
        kr, dr = oracle.orb_extract(right, p)
        obs, _ = S.stereo_match_ref(left, right, kl, dl, kr, dr)
        kept = obs["right_idx"] >= 0
        err = np.abs(obs["disparity"][kept] - d[np.clip(np.rint(kl["y"][kept]).astype(int), 0, H - 1)])
        return kept.mean(), (float(np.median(err)) if kept.any() else float("inf"))

    out = []
    for seed in (1, 2):
        raw_l, raw_r, d, left, right = R.raw_stereo_pair(seed, W, H, cal)
        out.append(dict(seed=seed, orig=chain(left, right, d), rect=chain(R.remap(raw_l, maps[0]), R.remap(raw_r, maps[1]), d),
                        raw=chain(raw_l, raw_r, d)))
    return out


def test_ref_accuracy_on_a_raw_synthetic_pair(accuracy):
    """raw_stereo_pair -> the restatement's remap -> oracle ORB -> stereo_ref at 320x240 / 500 features, against the same chain
    on the never-distorted pair and on the raw pair without rectification. Measured here (share matched, median |disparity
    error| in px): seed 1 original 0.717 / 0.010, rectified 0.727 / 0.148, raw 0.085 / 10.7; seed 2 original 0.660 / 0.017,
    rectified 0.692 / 0.112, raw 0.095 / 8.9."""
    for a in accuracy:
        print("seed %d: original %.3f / %.4f px, rectified %.3f / %.4f px, raw %.3f / %.4f px"
              % ((a["seed"],) + a["orig"] + a["rect"] + a["raw"]))
        assert a["rect"][0] >= a["orig"][0] - SHARE_MARGIN
        assert a["rect"][1] <= a["orig"][1] + MEDIAN_MARGIN
        assert a["raw"][0] < a["rect"][0]                          # what the feature is for
