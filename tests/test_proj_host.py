"""Guided matching (include/aria_orb_hip.h, "guided matching"): the parts that need no GPU -- exports, record layouts, defaults
and config validation, and the NumPy restatement (aria_slam_amd/proj_ref.py, which is the definition) on the written-down
answers of tests/proj_cases.py, against a literal triple loop, and on a hand-made arena."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_cases as PC   # noqa: E402
from aria_slam_amd import proj_ref as R   # noqa: E402

PROJ_SYMBOLS = ["aria_proj_default_config", "aria_proj_create", "aria_proj_destroy", "aria_proj_stream", "aria_proj_check",
                "aria_proj_search_batch_device", "aria_proj_search", "aria_proj_landmarks_from_map_device"]


def test_proj_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in PROJ_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipProjectionMatcher" in aria.__all__


def test_proj_record_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    assert (_lib.PROJ_LANDMARK_DTYPE.itemsize, _lib.PROJ_OBS_DTYPE.itemsize, _lib.PROJ_PAIR_DTYPE.itemsize) == (64, 24, 8)
    assert list(_lib.PROJ_LANDMARK_DTYPE.names) == ["X", "desc", "octave", "source"]
    assert list(_lib.PROJ_OBS_DTYPE.names) == ["u", "v", "kp_idx", "hamming", "second", "flags"]
    assert list(_lib.PROJ_PAIR_DTYPE.names) == ["landmark", "keypoint"]
    assert C.sizeof(_lib.ProjConfig) == 80
    cfg = _lib.ProjConfig()
    aria.load_library().aria_proj_default_config(C.byref(cfg))
    assert cfg.struct_size == 80 and not cfg.stream
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375)
    assert (cfg.min_depth, cfg.radius_px, cfg.th_hamming, cfg.max_octave_diff) == (0.1, 15.0, 100, 1)
    assert np.float32(cfg.ratio) == np.float32(0.9)
    d = R.DEFAULTS
    assert (d["K"], d["min_depth"], d["radius_px"], d["ratio"], d["th_hamming"], d["max_octave_diff"]) == (R.EUROC_K, 0.1, 15.0, 0.9, 100, 1)
    assert [np.float32(s) for _, _, _, s in aria.level_info(500, 320, 240)] == list(R.level_scales())


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("fx", 0.0), ("fy", -1.0), ("cx", float("nan")), ("cy", float("inf")),
                                         ("min_depth", float("nan")), ("radius_px", -1.0), ("radius_px", 2000.0),
                                         ("radius_px", float("nan")), ("ratio", -0.1), ("ratio", 1.5), ("ratio", float("nan")),
                                         ("th_hamming", -1), ("th_hamming", 258), ("max_octave_diff", -1), ("max_octave_diff", 9)])
def test_proj_create_refuses_a_bad_config_before_touching_a_device(aria, field, value):
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.ProjConfig()
    L.aria_proj_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_proj_create(C.byref(cfg), C.byref(h)) == -1 and not h      # ARIA_E_INVALID
    assert L.aria_proj_check(None) == -1 and L.aria_proj_stream(None) is None
    L.aria_proj_destroy(None)


def _frames():
    t = PC.table()
    return [pytest.param(f, id=f["name"]) for f in t["frames"]]


@pytest.mark.parametrize("f", _frames())
def test_restatement_equals_the_written_down_answers(f):
    t = PC.table()
    kp, desc = PC.frame_arrays(f)
    obs, corr, pairs, valid = R.search_frame_ref(f["pose"], kp, desc, f["n"], t["kp_stride"], t["landmarks"], f["first"], f["count"],
                                                 t["land_cap"], t["cfg"], t["width"], t["height"])
    want_obs, want_corr, want_pairs = PC.expected(f, t["landmarks"])
    assert valid == f["valid"]
    for name in obs.dtype.names:
        bad = np.flatnonzero(obs[name].view(np.int32) != want_obs[name].view(np.int32))
        assert len(bad) == 0, (f["name"], name, bad[:8], obs[name][bad[:8]], want_obs[name][bad[:8]])
    assert corr.tobytes() == want_corr.tobytes() and pairs.tobytes() == want_pairs.tobytes()
    assert np.isfinite(obs["u"]).all() and np.isfinite(obs["v"]).all()
    assert np.isfinite(corr["X"]).all() and np.isfinite(corr["u"]).all() and np.isfinite(corr["v"]).all()


def test_the_table_holds_every_case_of_the_issue():
    t = PC.table()
    frames = {f["name"]: f for f in t["frames"]}
    assert [len(frames[n]["kp"]) for n in ("grid 301", "grid 0", "grid 64")] == [301, 0, 64] and frames["grid 301"]["count"] == 130
    assert frames["grid 301"]["first"] == frames["grid 0"]["first"] == frames["grid 64"]["first"]          # one range, shared
    a, b = frames["grid 301"], frames["grid tail (overlapping range)"]
    assert a["first"] < b["first"] < a["first"] + a["count"] == b["first"] + b["count"]                    # ranges that overlap
    assert frames["count 0"]["count"] == 0 and frames["a range of one chunk + 1"]["count"] == PC.CHUNK + 1
    assert sum(not f["valid"] for f in t["frames"]) == 8
    for i, f in enumerate(t["frames"]):                                       # an invalid frame sits between valid neighbours
        if not f["valid"]:
            assert t["frames"][i - 1]["valid"] and t["frames"][i + 1]["valid"]
    flags = np.concatenate([f["exp"]["flags"] for f in t["frames"] if f["valid"]])
    assert {0, 1, 3, 7, 15} <= set(flags.tolist())


def test_brute_force_with_a_ratio_test_keeps_none_of_the_repeated_texture(oracle):
    """The case guided matching exists for: every landmark's descriptor occurs on two keypoints, so the two best distances of
    the brute-force matcher tie and Lowe's ratio at 0.75 drops all twelve; the window search matches all twelve."""
    t = PC.table()
    f = [f for f in t["frames"] if f["name"] == "repeated texture"][0]
    lm = t["landmarks"][f["first"]:f["first"] + f["count"]]
    got = oracle.match_ratio(np.ascontiguousarray(lm["desc"]), np.ascontiguousarray(f["desc"]), 0.75)
    assert len(got) == 0
    obs, corr, pairs = R.search_ref(f["pose"], f["kp"], f["desc"], lm, t["cfg"], t["width"], t["height"], first=f["first"])
    assert len(corr) == 12 and (obs["flags"] == 15).all() and sorted(pairs["keypoint"]) == list(range(12))


@pytest.mark.parametrize("name", ["window edges and image borders", "depth, dead landmarks, NaN and Inf",
                                  "ties, single candidates, thresholds", "two landmarks claim one keypoint",
                                  "octave differences and clamping", "repeated texture", "grid 64"])
def test_restatement_equals_a_literal_triple_loop(name):
    t = PC.table()
    f = [f for f in t["frames"] if f["name"] == name][0]
    lm = t["landmarks"][f["first"]:f["first"] + f["count"]]
    obs, _, _ = R.search_ref(f["pose"], f["kp"], f["desc"], lm, t["cfg"], t["width"], t["height"])
    loop = R.search_triple_loop(f["pose"], f["kp"], f["desc"], lm, t["cfg"], t["width"], t["height"])
    assert obs.tobytes() == loop.tobytes()


def test_triple_loop_on_random_crowded_scenes():
    """Many landmarks per keypoint and many keypoints per window, so ties, lost claims and ratio rejections all occur."""
    rng = np.random.default_rng(5)
    base = R.random_descriptors(rng, 6)
    seen = set()
    for trial in range(3):
        lms = np.concatenate([R.make_landmark(int(rng.integers(0, 64)), int(rng.integers(0, 48)), R.flip_bits(base[rng.integers(0, 6)], int(rng.integers(0, 3))),
                                              octave=int(rng.integers(-1, 4))) for _ in range(40)])
        kp = np.concatenate([R.make_keypoint(np.float32(rng.uniform(-5, 70)), np.float32(rng.uniform(-5, 55)), int(rng.integers(0, 5))) for _ in range(50)])
        desc = np.stack([R.flip_bits(base[rng.integers(0, 6)], int(rng.integers(0, 40)), start=int(rng.integers(0, 200))) for _ in range(50)])
        cfg = dict(K=R.EXACT_K, radius_px=6.0, ratio=0.95, th_hamming=60)
        obs, corr, pairs = R.search_ref(R.IDENTITY_POSE, kp, desc, lms, cfg, 64, 48)
        assert obs.tobytes() == R.search_triple_loop(R.IDENTITY_POSE, kp, desc, lms, cfg, 64, 48).tobytes()
        assert len(set(pairs["keypoint"].tolist())) == len(pairs)                 # a keypoint serves one landmark
        seen |= set(obs["flags"].tolist())
    assert {0, 1, 3, 7, 15} <= seen


def test_landmarks_from_map_ref_on_a_hand_made_arena():
    from aria_slam_amd._lib import KP_DTYPE, MAP_POINT_DTYPE
    rng = np.random.default_rng(9)
    n_slots, stride = 3, 8
    kp = np.zeros((n_slots, stride), KP_DTYPE)
    kp["octave"] = rng.integers(0, 8, (n_slots, stride))
    desc = R.random_descriptors(rng, n_slots * stride).reshape(n_slots, stride, 32)
    n = np.array([8, 5, 0], np.int32)
    arena = np.zeros(10, MAP_POINT_DTYPE)
    #            pair idx1 idx2
    rows = [(10, 0, 7), (10, 3, 0), (11, 1, 4), (11, 2, 5), (12, 0, 0), (9, 0, 0), (13, 0, 0), (10, 1, -1), (11, 7, 1), (10, 2, 2)]
    for j, (p, i1, i2) in enumerate(rows):
        arena[j]["pair"], arena[j]["idx1"], arena[j]["idx2"], arena[j]["X"] = p, i1, i2, (j + 0.5, -j, 2.0 * j)
    lm, cnt, invalid = R.landmarks_from_map_ref(arena, 9, 1, 12, 10, 2, kp, desc, n, stride, n_slots)   # positions 1..8 of a map of 9
    assert cnt == 8 and invalid and len(lm) == 12
    assert list(lm["source"]) == [1, 2, 3, 4, 5, 6, 7, 8, -1, -1, -1, -1]
    # view 2: position 1 -> slot 0 kp 0; 2 -> slot 1 kp 4; 3 -> slot 1 idx 5 >= n[1]: dead; 4 -> slot 2 is empty: dead; 5, 6: pair outside
    # the slots: dead; 7 -> idx2 = -1: dead; 8 -> slot 1 kp 1
    live = {0: (0, 0), 1: (1, 4), 7: (1, 1)}
    for j in range(12):
        if j in live:
            s, i = live[j]
            assert lm["octave"][j] == kp["octave"][s, i] and lm["desc"][j].tobytes() == desc[s, i].tobytes()
            assert lm["X"][j].tobytes() == arena["X"][1 + j].tobytes()
        else:
            assert lm["octave"][j] == -1 and not lm["desc"][j].any() and not lm["X"][j].any()
    lm1, cnt1, invalid1 = R.landmarks_from_map_ref(arena, 2, 0, 4, 10, 1, kp, desc, n, stride, n_slots)   # view 1, all in range
    assert cnt1 == 2 and not invalid1 and list(lm1["source"]) == [0, 1, -1, -1] and list(lm1["octave"][:2]) == [kp["octave"][0, 0], kp["octave"][0, 3]]
    assert R.landmarks_from_map_ref(arena, 3, 5, 4, 10, 1, kp, desc, n, stride, n_slots)[1] == 0           # first beyond the size


def test_proj_search_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "proj_search.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "proj_search.hip")).read()
    src += "".join(open(os.path.join(ROOT, "aria_slam_amd", "csrc", h)).read() for h in ("stage_handle.h", "ransac_device.h") if '#include "%s"' % h in src)
    assert "getenv" not in src
