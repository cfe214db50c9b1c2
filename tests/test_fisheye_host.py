"""The fisheye model KB4 of the rectification stage (include/aria_orb_hip.h, steps 2k and 4k): what needs no GPU. The
accuracy of rect_atan and rect_tan -- atan and tan from + - * / and sqrt -- against libm, the maps they give against the
same maps built with libm's atan, the invalid shares and the fold rule on the cases of fisheye_cases.py, both outcomes of
the points step and its round trip, agreement with the radtan model on a pinhole, the unchanged radtan camera dict, the
sensor.yaml reader, the model of a handle and the config validation."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisheye_cases as F   # noqa: E402
import rectify_cases as RC   # noqa: E402
from aria_slam_amd import rectify_ref as R   # noqa: E402


def test_rect_atan_against_libm():
    """300 k points of [0, 5] and of logspace(-12, 3). Bound 1e-13 absolute: at focal lengths up to 2047 px and 32 sub-steps
    per pixel that moves 32 su by at most 6.6e-9, under 0.004 expected flipped entries on the largest map tested here."""
    x = np.concatenate([np.linspace(0.0, 5.0, 300000), np.logspace(-12, 3, 300000)])
    want = np.array([math.atan(v) for v in x])
    err = np.abs(R.rect_atan(x) - want).max()
    print("rect_atan: largest absolute error %.3g" % err)
    assert err <= 1e-13
    assert R.rect_atan(0.0) == 0.0
    with np.errstate(all="ignore"):
        assert not np.isfinite(R.rect_atan(np.array([np.nan, np.inf]))).any()             # the pixel becomes invalid
    assert abs(float(R.rect_atan(1e150)) - math.pi / 2) <= 1e-13                          # below the overflow of t t (1.3e154)


def test_rect_tan_against_libm():
    """300 k points of [0, 1.5] rad. Bound 1e-12 relative, four orders below what the fp32 store resolves."""
    a = np.linspace(0.0, 1.5, 300000)
    want = np.array([math.tan(v) for v in a])
    got = R.rect_tan(a)
    err = np.abs(got[1:] - want[1:]) / want[1:]
    print("rect_tan: largest relative error %.3g" % err.max())
    assert got[0] == 0.0 and err.max() <= 1e-12


@pytest.mark.parametrize("new_K", F.WIDE_NEW_KS, ids=["newK=K", "newK=60"])
def test_wide_map_against_libm_atan(monkeypatch, new_K):
    """WIDE512, 262 144 entries: at most one entry may differ from the map built with math.atan, by one unit of qx or qy."""
    w, h = F.WIDE_SIZE
    got = R.build_map(F.WIDE512, new_K, w, h, w, h)
    monkeypatch.setattr(R, "rect_atan", lambda r: np.array([math.atan(v) for v in np.ravel(r)]).reshape(np.shape(r)))
    want = R.build_map(F.WIDE512, new_K, w, h, w, h)
    diff = np.flatnonzero(got != want)
    print("%d of %d entries differ, %.3f invalid" % (len(diff), got.size, (got == R.INVALID).mean()))
    assert len(diff) <= 1
    for i in diff:
        a, b = int(got.flat[i]), int(want.flat[i])
        assert a != R.INVALID and b != R.INVALID
        assert abs((a & 0xFFFF) - (b & 0xFFFF)) + abs((a >> 16) - (b >> 16)) == 1
    assert 0 < (got != R.INVALID).mean()


def _valid_without_fold(case):
    su, sv, Z = R.source_coords(case.cam, case.new_K, *case.dst)
    with np.errstate(all="ignore"):
        qx, qy = np.floor(su * 32.0 + 0.5), np.floor(sv * 32.0 + 0.5)
        return ((Z > 0) & np.isfinite(su) & np.isfinite(sv) & (qx >= 0) & (qy >= 0) & (qx < (case.src[0] - 1) * 32.0) &
                (qy < (case.src[1] - 1) * 32.0))


def test_case_shares_and_fold_counts():
    for name, share in F.INVALID_SHARE.items():
        case = F.CASES[name]
        got = (case.map == R.INVALID).mean()
        print("%s: %.3f invalid" % (name, got))
        assert abs(got - share) <= 0.03, name
    zoom, fold, yaw = F.CASES["zoom10"], F.CASES["fold8"], F.CASES["yaw75"]
    assert not R.fold_invalid(zoom.cam, zoom.new_K, *zoom.dst).any()                  # none by the fold rule
    folded = R.fold_invalid(fold.cam, fold.new_K, *fold.dst)
    assert folded.sum() == 544 and np.array_equal(folded, fold.map == R.INVALID)      # all of them by the fold rule ...
    assert _valid_without_fold(fold).all()                                            # ... alone: they would read the image
    assert (R.source_coords(yaw.cam, yaw.new_K, *yaw.dst)[2] <= 0).sum() > 50         # a camera that looks away
    rig = F.CASES["rig"]
    assert (rig.map != R.INVALID).mean() > 0.5
    # the remap cases reach both loaded read forms of k_rect_remap (counts: none 147, rows 255, taps 318 of 720 lanes)
    forms = zoom.forms["form"]
    assert (forms == RC.ROWS).sum() >= 50 and (forms == RC.TAPS).sum() >= 50 and (forms == RC.NONE).sum() >= 50


def test_points_have_both_outcomes_and_round_trip():
    kp = F.keypoints()
    for name, cam in F.point_cameras():
        want = F.ref_points_all()[name]
        gone = valid = 0
        for f, n in enumerate(F.POINT_COUNTS):
            g = (want[f, :n]["x"] == -1) & (want[f, :n]["y"] == -1)
            assert g.any() and (~g).any(), (name, f)
            assert g[RC.POINT_NONFINITE].all()
            gone, valid = gone + int(g.sum()), valid + int((~g).sum())
        print("%s: %d valid, %d invalid" % (name, valid, gone))
        assert valid >= 50 and gone >= 50, name
        assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()          # no NaN or Inf is ever written
        if cam["R"] != R.IDENTITY:
            continue
        # distort(undistort) on the valid points, fp64 end to end (R = I, new K = K)
        p = np.stack([kp[1]["x"], kp[1]["y"]], axis=1).astype(np.float64)
        u = R.undistort_points(p, cam, cam["K"])
        ok = ~((u[:, 0] == -1) & (u[:, 1] == -1))
        back = R.distort(u[ok], cam)
        err = np.abs(back - p[ok]).max()
        print("%s: round trip of %d points within %.3g px" % (name, int(ok.sum()), err))
        assert ok.sum() >= 25 and err <= 1e-9


def test_models_agree_on_a_pinhole():
    """All k zero, R = I: the kb4 map equals the radtan map with zero coefficients but for entries within one unit, at most 1
    per 1000 of them -- where the camera IS a pinhole. KB4 with k = 0 is the equidistant lens (image radius f a, a the angle
    from the axis), the radtan model with zero coefficients the pinhole (f tan a); they are one camera in the paraxial limit
    only, so the case is a focal length at which the whole image is paraxial. A source pixel r px from the principal point
    moves by f (tan a - a) <= r^3 / (3 f^2) px; with r <= 70 px (the corner of the 96x64 source seen at zoom 0.93) and f =
    2e5 px that is 2.9e-6 px = 9.1e-5 units of 1/32 px per axis, so at most 6144 * 2 * 9.1e-5 = 1.1 entries are expected to
    round the other way, against the 6.1 allowed. What is left to differ is everything else the two map kernels share and
    could get wrong: the ray, K, the rounding, the bounds, and rect_atan(r) / r -> 1. (At camera A's 36 px the same count is
    6089 of 6144, by up to 915 units: test_zero_coefficients_are_the_equidistant_lens.)"""
    K, new_K, src = F.K_TELE, F.TELE_NEW_K, F.SRC                                     # fisheye_cases' case "tele"
    a = F.CASES["tele"].map
    assert F.TELE == R.camera(K, (0.0,) * 4, model="kb4") and F.CASES["tele"].new_K == new_K
    b = R.build_map(R.camera(K), new_K, src[0], src[1], src[0], src[1])
    both = (a != R.INVALID) & (b != R.INVALID)
    ai, bi = a[both].astype(np.int64), b[both].astype(np.int64)
    step = np.abs((ai & 0xFFFF) - (bi & 0xFFFF)) + np.abs((ai >> 16) - (bi >> 16))
    differ = int((a != b).sum())
    print("%d of %d entries differ, by up to %d units; %.3f valid in both" % (differ, a.size, int(step.max()), both.mean()))
    assert step.max() <= 1 and differ <= a.size / 1000.0
    assert both.mean() > 0.5 and len(np.unique(ai & 31)) == 32 and len(np.unique((ai >> 16) & 31)) == 32


def test_zero_coefficients_are_the_equidistant_lens():
    """All k zero, R = I: a destination pixel at angle a from the axis reads the source at radius f a along the same
    direction, and the pixel on the axis reads the principal point -- there, and only there, the kb4 and the radtan map with
    zero coefficients agree. Bound: su is exact to a few ulp of 96 (1e-13), the map rounds to 1/32 px: half a unit plus that."""
    K = (36.0, 36.0, 47.0, 31.0)                                                      # the axis falls on a pixel
    w, h = F.SRC
    m = R.build_map(R.camera(K, (0.0,) * 4, model="kb4"), K, w, h, w, h)
    assert (m != R.INVALID).all()
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = (u - K[2]) / K[0], (v - K[3]) / K[1]
    r = np.hypot(x, y)
    sc = np.where(r == 0, 1.0, np.arctan(r) / np.where(r == 0, 1.0, r))
    qx, qy = (m & 0xFFFF).astype(np.float64), (m >> 16).astype(np.float64)
    assert np.abs(qx - 32.0 * (K[0] * x * sc + K[2])).max() <= 0.5 + 1e-9
    assert np.abs(qy - 32.0 * (K[1] * y * sc + K[3])).max() <= 0.5 + 1e-9
    pin = R.build_map(R.camera(K), K, w, h, w, h)
    assert m[31, 47] == pin[31, 47] == (47 * 32) | ((31 * 32) << 16)
    assert m[31, 90] != pin[31, 90]                                                   # 50 degrees off the axis they do not


def test_radtan_camera_is_what_it_was():
    want = dict(K=RC.K_L, dist=RC.D_L + (0.0,), R=R.IDENTITY)
    assert R.camera(RC.K_L, RC.D_L) == want and R.camera(RC.K_L, RC.D_L, model="radtan") == want
    assert R.camera((2.0, 2.0, 0.5, 0.5)) == dict(K=(2.0, 2.0, 0.5, 0.5), dist=(0.0,) * 5, R=R.IDENTITY)
    assert R.model_of(want) == "radtan"
    with pytest.raises(ValueError):
        R.camera(RC.K_L, (0.0,) * 6)
    k = R.camera(F.K_A, F.D_A, model="kb4")
    assert k == dict(K=F.K_A, dist=F.D_A + (0.0,), R=R.IDENTITY, model="kb4") and R.model_of(k) == "kb4"
    for bad in ((0.1,) * 5, (0.1,) * 3, ()):
        with pytest.raises(ValueError):
            R.camera(F.K_A, bad, model="kb4")
    with pytest.raises(ValueError):
        R.camera(F.K_A, F.D_A, model="kb3")
    cl, cr, _, _ = R.rectified_cameras(F.RIG)
    assert cl["model"] == cr["model"] == "kb4"
    assert "model" not in R.rectified_cameras(RC.EUROC)[0]


def test_sensor_yaml_reader(aria, tmp_path):
    path = str(tmp_path / "sensor.yaml")
    for name in ("equidistant", "fisheye", "kb4"):
        F.write_sensor_yaml(path, F.K_A, F.D_A, RC.T_BS_L, F.SRC, name)
        with pytest.raises(ValueError):
            aria.load_sensor_yaml(path)                                               # the default reader is radtan only
        cal = aria.load_sensor_yaml(path, fisheye=True)
        assert cal["model"] == "kb4" and cal["K"] == F.K_A and cal["dist"] == F.D_A + (0.0,)
        assert cal["resolution"] == F.SRC and np.array_equal(cal["T_BS"].reshape(-1), RC.T_BS_L)
    for coefficients in (F.D_A + (0.001,), F.D_A[:3]):
        F.write_sensor_yaml(path, F.K_A, coefficients, RC.T_BS_L, F.SRC)
        with pytest.raises(ValueError):
            aria.load_sensor_yaml(path, fisheye=True)
    RC.write_sensor_yaml(path, RC.K_L, RC.D_L, RC.T_BS_L)                             # a radtan file reads as before
    a, b = aria.load_sensor_yaml(path, fisheye=True), aria.load_sensor_yaml(path)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert aria.load_sensor_yaml(path)["model"] == "radial-tangential"


def test_mixed_models_raise(aria):
    """Refused in Python, before a handle or a device is touched."""
    radtan = R.camera(F.K_A, (0.01, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        aria.HipRectifier([F.A, radtan], new_K=F.K_A, src_size=F.SRC)
    with pytest.raises(ValueError):
        aria.HipRectifier([F.A, F.A], new_K=F.K_A, src_size=F.SRC, model="radtan")
    with pytest.raises(ValueError):
        aria.HipRectifier(F.A, new_K=F.K_A, src_size=F.SRC, model="kb3")
    with pytest.raises(ValueError):
        aria.HipRectifier.from_stereo_calibration(F.K_A, F.D_A + (0.0,), RC.T_BS_L, F.K_A, F.D_A, RC.T_BS_R, F.SRC, model="kb4")


def test_config_model_word(aria):
    """reserved became model: same layout, 0 by default, anything but 0 and 1 refused, KB4 with dist[4] != 0 refused -- all
    before any device is touched."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    assert C.sizeof(_lib.RectConfig) == 368 and _lib.RectConfig.model.offset == 364
    assert (_lib.RECT_MODEL_RADTAN, _lib.RECT_MODEL_KB4) == (0, 1) and R.MODELS == ("radtan", "kb4")
    cfg = _lib.RectConfig()
    cfg.model = 7
    L.aria_rect_default_config(C.byref(cfg))
    assert cfg.model == 0
    h = C.c_void_p()
    for model in (2, -1, 256):
        cfg.model = model
        assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    cfg.model = _lib.RECT_MODEL_KB4
    cfg.cam[0].dist[:] = list(F.D_A) + [1e-300]
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    cfg.n_cameras = 2                                                                  # the second camera is checked too
    cfg.cam[0].dist[4] = 0.0
    cfg.cam[1].dist[:] = list(F.D_A) + [0.5]
    assert L.aria_rect_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
