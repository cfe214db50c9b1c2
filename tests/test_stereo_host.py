"""Sparse stereo (include/aria_orb_hip.h, "sparse stereo"): the parts that need no GPU -- exports, record layouts, defaults and
config validation, the NumPy restatement (aria_slam_amd/stereo_ref.py, which is the definition) on hand-made known answers
with one case per rule, its accuracy on the synthetic rectified scene, the scale restatement on exact depths, and the
kernels' listing."""
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
import stereo_cases   # noqa: E402

STEREO_SYMBOLS = ["aria_stereo_default_config", "aria_stereo_create", "aria_stereo_destroy", "aria_stereo_stream",
                  "aria_stereo_check", "aria_stereo_match_batch_device", "aria_stereo_match", "aria_stereo_scale_batch_device",
                  "aria_stereo_scale_pose"]


def test_stereo_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in STEREO_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipStereoMatcher" in aria.__all__


def test_stereo_record_layouts_and_defaults(aria):
    from aria_slam_amd import _lib, stereo_ref
    assert _lib.STEREO_OBS_DTYPE.itemsize == 32 and _lib.STEREO_SCALE_DTYPE.itemsize == 16
    assert list(_lib.STEREO_OBS_DTYPE.names) == ["u_right", "disparity", "depth", "X", "Y", "right_idx", "hamming", "sad"]
    assert C.sizeof(_lib.StereoConfig) == 112
    cfg = _lib.StereoConfig()
    aria.load_library().aria_stereo_default_config(C.byref(cfg))
    assert cfg.struct_size == 112 and not cfg.stream
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375)
    assert (cfg.baseline, cfg.min_disparity, cfg.max_disparity) == (0.110, 0.0, 458.654)
    assert (cfg.th_hamming, cfg.sad_half_window, cfg.sad_slide, cfg.max_octave_diff, cfg.min_scale_matches) == (75, 5, 5, 1, 5)
    assert (cfg.band_factor, cfg.median_factor) == (2.0, 2.1)
    d = stereo_ref.DEFAULTS
    assert (d["baseline"], d["th_hamming"], d["sad_half_window"], d["sad_slide"], d["band_factor"], d["max_octave_diff"],
            d["median_factor"], d["min_scale_matches"]) == (0.110, 75, 5, 5, 2.0, 1, 2.1, 5)
    # scale[o] of the restatement is aria_orb_level_info's
    assert [np.float32(s) for _, _, _, s in aria.level_info(500, 320, 240)] == list(stereo_ref.level_scales())


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("fx", 0.0), ("fy", -1.0), ("cx", float("nan")),
                                         ("baseline", 0.0), ("baseline", float("inf")), ("max_disparity", 0.0),
                                         ("min_disparity", 500.0), ("band_factor", -1.0), ("median_factor", float("nan")),
                                         ("th_hamming", -1), ("sad_half_window", 0), ("sad_half_window", 8), ("sad_slide", 0),
                                         ("sad_slide", 17), ("max_octave_diff", -1), ("min_scale_matches", 0)])
def test_stereo_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.StereoConfig()
    L.aria_stereo_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_stereo_create(C.byref(cfg), C.byref(h)) == -1      # ARIA_E_INVALID
    assert not h.value
    assert L.aria_stereo_create(None, C.byref(h)) == -1
    assert L.aria_stereo_check(None) == -1


@pytest.fixture(scope="module")
def rule_results():
    from aria_slam_amd import stereo_ref as R
    out = {}
    for c in stereo_cases.rule_cases():
        obs, m = R.stereo_match_ref(c["img_l"], c["img_r"], c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **c["cfg"])
        out[c["name"]] = (c, obs, m)
    return out


def _check_expect(c, obs, m):
    from aria_slam_amd import stereo_ref as R
    assert len(obs) == len(c["expect"])
    none = R.unmatched_obs(1)[0]
    kept = []
    for i, e in enumerate(c["expect"]):
        if e is None:
            assert obs[i] == none, (c["name"], i, obs[i])
        else:
            assert obs[i]["right_idx"] == e[0], (c["name"], i, obs[i])
            kept.append(i)
    assert list(m["query_idx"]) == kept and list(m["train_idx"]) == [c["expect"][i][0] for i in kept]
    assert np.array_equal(m["distance"], obs["hamming"][kept].astype(np.float32))
    assert np.isfinite(np.stack([obs[f] for f in ("u_right", "disparity", "depth", "X", "Y")])).all()


def test_ref_candidate_rules(rule_results):
    """Duplicate descriptors -> lowest j; |dy| exactly on the band accepted, beyond it excluded; octave difference 2 excluded,
    1 accepted; both x bounds inclusive, one ulp beyond excluded; a best SAD of 1 beside zeros (med = 0) is dropped while
    the zeros stay."""
    from aria_slam_amd import stereo_ref as R
    c, obs, m = rule_results["candidates"]
    _check_expect(c, obs, m)
    best, dist = R.best_candidates(c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **c["cfg"])
    assert list(best) == [0, 2, -1, -1, 5, 6, 7, -1, 9] and (dist[best >= 0] == 0).all()
    # the window sits on integer shifts of an exact copy: SAD 0, sub-pixel offset below half a pixel
    for i, e in enumerate(c["expect"]):
        if e is not None:
            assert obs[i]["sad"] == 0 and obs[i]["hamming"] == 0 and abs(obs[i]["disparity"] - e[1]) <= 0.5
            assert obs[i]["u_right"] == c["kp_l"]["x"][i] - obs[i]["disparity"]
    # keypoint 8 reached step 4 with SAD 1 and fell to the strict median rule (med = 0); alone in its pair (med = 1) it stays
    obs2, _ = R.stereo_match_ref(c["img_l"], c["img_r"], c["kp_l"][8:], c["desc_l"][8:], c["kp_r"], c["desc_r"], **c["cfg"])
    assert obs2[0]["right_idx"] == 9 and obs2[0]["sad"] == 1 and abs(obs2[0]["disparity"] - 10.0) <= 0.5


def test_ref_slide_rules(rule_results):
    """Left window off the image, both off at the top, the right slide off on the left; best inc at -L and at +L; flat
    texture. den == 0 itself cannot be reached: the best inc is a strict minimum towards lower incs and a minimum towards
    higher ones, so d1 > d2 <= d3 and den = 2 (d1 + d3 - 2 d2) > 0 -- a flat window is rejected by the end-of-slide rule."""
    from aria_slam_amd import stereo_ref as R
    c, obs, m = rule_results["slide"]
    _check_expect(c, obs, m)
    w, L = 5, 5
    assert R.sad_slide(c["img_l"], c["img_r"], 92, 30, 82, w, L) is None
    assert R.sad_slide(c["img_l"], c["img_r"], 70, 3, 60, w, L) is None
    assert R.sad_slide(c["img_l"], c["img_r"], 19, 56, 9, w, L) is None
    assert int(np.argmin(R.sad_slide(c["img_l"], c["img_r"], 80, 30, 75, w, L))) == 0
    assert int(np.argmin(R.sad_slide(c["img_l"], c["img_r"], 80, 42, 65, w, L))) == 2 * L
    assert not R.sad_slide(c["img_l"], c["img_r"], 30, 30, 20, w, L).any()
    assert abs(obs[6]["disparity"] - 10.0) <= 0.5


def test_ref_clamp_and_empty_sides(rule_results):
    from aria_slam_amd import stereo_ref as R
    c, obs, m = rule_results["clamp"]
    _check_expect(c, obs, m)
    fx, cx = np.float32(R.EUROC_K[0]), np.float32(R.EUROC_K[2])
    depth = fx * np.float32(0.110) / np.float32(0.01)
    assert obs[0]["disparity"] == np.float32(0.01) and obs[0]["depth"] == depth and obs[0]["sad"] == 0
    assert obs[0]["u_right"] == np.float32(48.0) - np.float32(0.01)
    assert obs[0]["X"] == (np.float32(48.0) - cx) * depth / fx
    for name in ("empty_right", "empty_left"):
        c, obs, m = rule_results[name]
        _check_expect(c, obs, m)
        assert len(m) == 0


@pytest.fixture(scope="module")
def scene_results(oracle):
    from aria_slam_amd import stereo_ref as R
    out = []
    for seed in (1, 2):
        left, right, d = R.stereo_pair(seed, 320, 240)
        p = oracle.default_params(500)
        kl, dl = oracle.orb_extract(left, p)
        kr, dr = oracle.orb_extract(right, p)
        obs, m = R.stereo_match_ref(left, right, kl, dl, kr, dr)
        out.append((seed, kl, obs, m, d))
    return out


def test_ref_accuracy_on_the_synthetic_scene(scene_results):
    """Seeds 1 and 2 at 320x240 / 500 features, extraction by the oracle. Measured here: 335 of 467 and 307 of 465 left
    keypoints kept, 98.5 % and 99.0 % of them within 0.5 px of the true row disparity, 100 % within 1 px."""
    for seed, kl, obs, m, d in scene_results:
        kept = obs["right_idx"] >= 0
        err = np.abs(obs["disparity"][kept] - d[np.rint(kl["y"][kept]).astype(int)])
        print("seed %d: kept %d of %d (%.1f %%), within 0.5 px %.1f %%, within 1 px %.1f %%"
              % (seed, kept.sum(), len(kl), 100 * kept.mean(), 100 * (err <= 0.5).mean(), 100 * (err <= 1.0).mean()))
        assert kept.mean() >= 0.60
        assert (err <= 0.5).mean() >= 0.95
        assert (err <= 1.0).mean() >= 0.99
        assert len(m) == kept.sum() and np.array_equal(m["query_idx"], np.flatnonzero(kept))
        assert np.isfinite(obs["depth"]).all() and (obs["depth"][kept] > 0).all()


def _scale_scene(n=200, seed=3, scale=2.5):
    """A two-view scene whose camera-frame points are exact in fp32: map_ref.synth_scene's points snapped to a 1/64 grid,
    R a quarter turn about z, t = (0.6, 0.8, 0), |t| = 1, true translation scale * t = (1.5, 2.0, 0)."""
    from aria_slam_amd import map_ref as M
    from aria_slam_amd import stereo_ref as R
    E = M.extrinsics(np.eye(3), [0, 0, 0])
    _, _, m, X1, _ = M.synth_scene(seed, n, E, M.extrinsics(np.eye(3), [-0.5, 0, 0]), noise_px=0.0)
    X1 = np.round(X1 * 64) / 64
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    t = np.array([0.6, 0.8, 0.0])
    X2 = X1 @ Rz.T + scale * t
    obs = []
    for X in (X1, X2):
        assert np.array_equal(X, X.astype(np.float32))
        o = R.unmatched_obs(n)
        o["X"], o["Y"], o["depth"], o["right_idx"] = X[:, 0], X[:, 1], X[:, 2], np.arange(n)
        obs.append(o)
    return (Rz, t, 1), m, obs[0], obs[1]


def test_scale_ref_recovers_the_true_translation_length():
    from aria_slam_amd import stereo_ref as R
    pose, m, o1, o2 = _scale_scene()
    r = R.stereo_scale_ref(pose, None, m, o1, o2)
    assert r["valid"] == 1 and r["n_used"] == 200 and abs(r["scale"] - 2.5) / 2.5 < 1e-9
    # swapped roles: view 1 is the train side
    sw = m.copy()
    sw["query_idx"], sw["train_idx"] = m["train_idx"], m["query_idx"]
    r2 = R.stereo_scale_ref(pose, None, sw, o2, o1, query_is_first=False)
    assert r2 == r
    # the mask and unmatched observations take matches out; outliers below half do not move the median
    mask = np.zeros(200, np.uint8)
    mask[::2] = 1
    o1b = o1.copy()
    o1b[:10] = R.unmatched_obs(1)[0]
    o2b = o2.copy()
    o2b["depth"][20:60] += 3.0
    r = R.stereo_scale_ref(pose, mask, m, o1b, o2b)
    assert r["valid"] == 1 and r["n_used"] == 95 and abs(r["scale"] - 2.5) / 2.5 < 1e-9
    # invalid pose record, too few matches, non-positive scale
    assert tuple(R.stereo_scale_ref((pose[0], pose[1], 0), None, m, o1, o2).tolist()) == (1.0, 0, 0)
    assert tuple(R.stereo_scale_ref(pose, None, m[:4], o1, o2).tolist()) == (1.0, 4, 0)
    assert tuple(R.stereo_scale_ref(pose, None, m[:5], o1, o2, min_scale_matches=5).tolist())[1:] == (5, 1)
    assert tuple(R.stereo_scale_ref((pose[0], -pose[1], 1), None, m, o1, o2).tolist()) == (1.0, 200, 0)


def test_stereo_kernels_cross_compile_without_scratch():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "stereo_match.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path, os.path.join(csrc, "stereo_match.hip")])
    text = open(path).read()
    for k in ("k_stereo_match", "k_stereo_scale"):
        body, meta = S.kernel_body(text, k)
        assert len(body) > 20, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        hist, _, _ = S.stats(body)
        assert not any(op.startswith("global_atomic") and ("f32" in op or "f64" in op) for op in hist), k   # no float atomics
        assert not any(op.startswith(("v_fma_f64", "v_fmac_f64")) for op in hist), k                        # no contraction
    hist, _, _ = S.stats(S.kernel_body(text, "k_stereo_match")[0])
    assert hist["v_sad_u8"] >= 4                                     # the slide is byte SAD on dwords
    assert hist["v_div_fixup_f32"] == 4                              # delta, depth, X, Y: correctly rounded divisions


def test_stereo_match_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "stereo_match.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "stereo_match.hip")).read()
    # the rules below follow the code into the shared headers this file includes
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in src)
    assert "getenv" not in src


def test_host_adapters_build_with_stereo_and_the_reader_pairs_cam1(aria, tmp_path):
    """libaria_hip_adapters.so holds HipStereoMatcher, euroc_frontend knows --stereo, and AslSequence pairs mav0/cam1 with cam0
    by equal timestamp; a tree without cam1 loads as before."""
    from test_frontend_io import write_png
    pkg = os.path.join(ROOT, "aria_slam_amd")
    subprocess.check_call(["make", "-C", os.path.join(pkg, "host"), "-s"])
    syms = subprocess.run(["nm", "-DC", os.path.join(pkg, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipStereoMatcher::match", "aria::adapters::hip::HipStereoMatcher::scale",
                 "aria::adapters::hip::StereoObservations::medianDepth", "aria::io::AslSequence::readRight"):
        assert name in syms, name
    usage = subprocess.run([os.path.join(pkg, "euroc_frontend")], capture_output=True, text=True)
    assert "--stereo" in usage.stderr and "--stereo-out" in usage.stderr
    L = C.CDLL(os.path.join(pkg, "libaria_hip_adapters.so"))
    L.aria_asl_stereo.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    L.aria_asl_list.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    img = np.arange(16 * 16, dtype=np.uint8).reshape(16, 16)
    t0 = 1403636579763555584
    stamps = [t0 + k * 50_000_000 for k in range(4)]
    for cam, rows in (("cam0", stamps), ("cam1", [stamps[3], stamps[1], stamps[0] + 25_000_000, stamps[0]])):   # no partner for frame 2
        d = tmp_path / "mav0" / cam / "data"
        d.mkdir(parents=True)
        for ts in rows:
            (d / ("%d.png" % ts)).write_bytes(write_png(img))
        (tmp_path / "mav0" / cam / "data.csv").write_text("#timestamp [ns],filename\n" + "".join("%d,%d.png\n" % (t, t) for t in rows))
    has = np.full(8, -1, np.int32)
    assert L.aria_asl_stereo(str(tmp_path).encode(), has.ctypes.data, 8) == 4
    assert list(has[:4]) == [1, 1, 0, 1]
    # without cam1: the same listing, no partners
    ts_a, ts_b = np.zeros(8), np.zeros(8)
    assert L.aria_asl_list(str(tmp_path).encode(), ts_a.ctypes.data, 8, None, 0) == 4
    import shutil
    shutil.rmtree(tmp_path / "mav0" / "cam1")
    assert L.aria_asl_list(str(tmp_path).encode(), ts_b.ctypes.data, 8, None, 0) == 4 and np.array_equal(ts_a, ts_b)
    assert L.aria_asl_stereo(str(tmp_path).encode(), has.ctypes.data, 8) == 4 and list(has[:4]) == [0, 0, 0, 0]
