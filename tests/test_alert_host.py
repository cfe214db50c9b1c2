"""Obstacle alerts (include/aria_orb_hip.h, "obstacle alerts"): the parts that need no GPU -- exports, layouts, defaults and
validation, the zone boundaries, and the NumPy restatement (aria_slam_amd/alert_ref.py, which is the definition) on known
answers: the order statistic against a literal sort, the sketch's own test case (H16:529-532), every priority boundary, and
a hand-written timeline of the cooldown rule."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_cases as AC   # noqa: E402
from aria_slam_amd import alert_ref as R   # noqa: E402

ALERT_SYMBOLS = ["aria_alert_default_config", "aria_alert_create", "aria_alert_destroy", "aria_alert_stream", "aria_alert_check",
                 "aria_alert_dets_seen", "aria_alert_measure_batch_device", "aria_alert_arbitrate_batch_device",
                 "aria_alert_run_batch_device", "aria_alert_measure", "aria_alert_arbitrate", "aria_alert_run", "aria_alert_zone_bounds",
                 "aria_alert_algorithmic_bytes"]
f32 = np.float32
MS = AC.MS


def test_alert_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in ALERT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipObstacleAlerter" in aria.__all__
    for words in ("sound synthesis and TTS", "traffic-light and sign classification", "tracking of objects across frames",
                  "BEHIND", "alerts from the volume or the plan", "tuning of the defaults", "H16_AUDIO_FEEDBACK.md:393-493",
                  "IAudioFeedback.hpp:7-78"):
        assert words in header, words


def test_alert_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    assert C.sizeof(_lib.AlertConfig) == 264
    assert _lib.ALERT_MEAS_DTYPE.itemsize == 16 and _lib.ALERT_MEAS_DTYPE == R.MEAS_DTYPE
    assert _lib.ALERT_EVENT_DTYPE.itemsize == 32 and _lib.ALERT_EVENT_DTYPE == R.EVENT_DTYPE
    assert _lib.ALERT_STATE_DTYPE.itemsize == 2320 and _lib.ALERT_STATE_DTYPE == R.STATE_DTYPE
    assert _lib.DETECTION_DTYPE == R.DETECTION_DTYPE and R.DETECTION_DTYPE.itemsize == 24
    assert not R.new_state(2).tobytes().strip(b"\0") and aria.HipObstacleAlerter.new_state(2).tobytes() == R.new_state(2).tobytes()
    cfg = _lib.AlertConfig()
    L.aria_alert_default_config(C.byref(cfg))
    d = R.config()
    assert cfg.struct_size == 264 and not cfg.stream
    assert (cfg.width, cfg.height, cfg.zone_top, cfg.zone_bottom) == (752, 480, 120, 480) == (d.width, d.height, d.zone_top, d.zone_bottom)
    assert (cfg.max_dets, cfg.min_valid) == (32, 16) == (d.max_dets, d.min_valid)
    assert (cfg.min_depth, cfg.max_depth) == (f32(0.1), f32(20.0)) == (d.min_depth, d.max_depth)
    assert ((cfg.zone_pct_num, cfg.zone_pct_den), (cfg.det_pct_num, cfg.det_pct_den)) == ((5, 100), (1, 2)) == (d.zone_pct, d.det_pct)
    assert (cfg.zone_alert_m, cfg.default_depth, cfg.crit_m, cfg.high_m, cfg.medium_m, cfg.beep_m) == (3.0, 5.0, 1.0, 2.0, 3.0, 1.5)
    assert (d.zone_alert_m, d.default_depth, d.crit_m, d.high_m, d.medium_m, d.beep_m) == (3.0, 5.0, 1.0, 2.0, 3.0, 1.5)
    assert cfg.obstacle_dangerous == 1 == d.obstacle_dangerous and tuple(cfg.dangerous[:cfg.n_dangerous]) == (0, 1, 2, 3, 5, 7) == d.dangerous
    assert cfg.max_events_per_frame == 2 == d.max_events_per_frame
    assert tuple(cfg.cooldown_ns) == (2000 * MS, 800 * MS, 500 * MS, 0) == d.cooldown_ns
    assert (R.LOW, R.MEDIUM, R.HIGH, R.CRITICAL) == (0, 1, 2, 3) and (R.CENTER, R.LEFT, R.RIGHT) == (0, 1, 2)    # the reference's enums
    assert L.aria_alert_algorithmic_bytes(752, 120, 480, 1) == 4 * 752 * 360 + 16 * 64
    assert L.aria_alert_algorithmic_bytes(752, 120, 120, 1) == -1 and L.aria_alert_algorithmic_bytes(0, 0, 1, 1) == -1
    assert L.aria_alert_check(None) == -1 and L.aria_alert_dets_seen(None) == -1
    assert L.aria_alert_measure_batch_device(None, None, 0, 0, 0, None, None, 0, None) == -1


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("width", 0), ("width", 8193), ("height", 0), ("zone_top", -1),
                                         ("zone_top", 480), ("zone_bottom", 120), ("zone_bottom", 481), ("max_dets", 62), ("max_dets", -1),
                                         ("min_valid", 0), ("min_depth", 0.0), ("min_depth", float("nan")), ("max_depth", 0.05),
                                         ("max_depth", float("inf")), ("zone_pct_num", 100), ("zone_pct_num", -1), ("det_pct_num", 2),
                                         ("det_pct_den", 0), ("zone_alert_m", float("nan")), ("default_depth", float("inf")),
                                         ("n_dangerous", 33), ("max_events_per_frame", 65), ("max_events_per_frame", -1)])
def test_alert_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched (device 99 is never reached), and the restatement refuses
    the same."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.AlertConfig()
    L.aria_alert_default_config(C.byref(cfg))
    cfg.device = 99
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_alert_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    ref = {"zone_pct_num": dict(zone_pct=(value, 100)), "det_pct_num": dict(det_pct=(value, 2)), "det_pct_den": dict(det_pct=(1, value)),
           "n_dangerous": dict(dangerous=tuple(range(33))), "struct_size": None}.get(field, {field: value})
    if ref is not None:
        assert not R.valid_config(R.config(**ref))
    assert R.valid_config(R.config())
    cfg = _lib.AlertConfig()
    L.aria_alert_default_config(C.byref(cfg))
    cfg.cooldown_ns[2] = -1
    assert L.aria_alert_create(C.byref(cfg), C.byref(h)) == -1 and not R.valid_config(R.config(cooldown_ns=(0, 0, -1, 0)))


@pytest.mark.parametrize("width", [1, 3, 20, 37, 640, 752])
def test_zone_bounds_are_the_per_column_float_test(aria, width):
    b0, b1 = aria.HipObstacleAlerter.zone_bounds(width)
    zones = []
    for x in range(width):
        v = (f32(x) + f32(0.5)) / f32(width)
        assert v.dtype == np.float32
        zones.append(R.LEFT if v < f32(0.35) else R.RIGHT if v > f32(0.65) else R.CENTER)
    assert zones == [R.LEFT] * b0 + [R.CENTER] * (b1 - b0) + [R.RIGHT] * (width - b1)
    assert (b0, b1) == R.zone_bounds(width)
    print(width, b0, b1)
    assert aria.load_library().aria_alert_zone_bounds(0, (C.c_int * 2)()) == -1


def test_zone_bounds_known():
    assert R.zone_bounds(1) == (0, 1) and R.zone_bounds(3) == (1, 2) and R.zone_bounds(20) == (7, 13)
    assert R.zone_bounds(752) == (263, 489) and R.zone_bounds(640) == (224, 416)


def test_order_statistic_against_a_literal_sort():
    rng = np.random.default_rng(11)
    c = R.config(min_valid=4)
    for n in (3, 4, 5, 64, 1000):
        v = rng.uniform(-1, 25, n).astype(np.float32)
        v[rng.random(n) < 0.2] = np.nan
        good = sorted(float(x) for x in v if 0.1 <= x <= 20.0)
        for pct in ((5, 100), (1, 2), (0, 1), (99, 100)):
            dist, nv, k, flags = R.order_statistic(v, c, pct)
            assert nv == len(good)
            if nv < 4:
                assert (dist, k, flags) == (-1.0, 0, R.MEAS_SOURCE)
            else:
                assert k == nv * pct[0] // pct[1] and float(dist) == good[k] and flags == R.MEAS_SOURCE | R.MEAS_OK
    # the edges of the valid range are valid; one ulp outside is not
    e = np.array([0.1, 20.0, np.nextafter(f32(0.1), f32(0)), np.nextafter(f32(20.0), f32(30))], np.float32)
    assert R.order_statistic(e, R.config(min_valid=1), (0, 1))[:2] == (f32(0.1), 2)


def test_rectangles():
    c = R.config(width=100, height=50, zone_top=10, zone_bottom=40)
    D = AC.det
    rect = lambda *a: R.source_rect(c, 3, np.array(D(*a), R.DETECTION_DTYPE))   # noqa: E731
    assert R.source_rect(c, 0) == (35, 10, 65, 40) and R.source_rect(c, 1) == (0, 10, 35, 40) and R.source_rect(c, 2) == (65, 10, 100, 40)
    assert rect(10.9, 5.2, 20.9, 9.9) == (10, 5, 20, 9)                 # (int): truncation
    assert rect(-0.9, -3.5, 200, 200) == (0, 0, 100, 50)
    assert rect(np.nan, 0, 5, 5) == (0, 0, 0, 0) and rect(0, 0, np.inf, 5) == (0, 0, 0, 0)
    assert rect(0, 0, 2.0 ** 20, 5) == (0, 0, 100, 5) and rect(0, 0, 2.0 ** 20 + 1, 5) == (0, 0, 0, 0)
    assert R.det_count(5, 8, 3) == (3, False) and R.det_count(9, 8, 3) == (0, True) and R.det_count(-1, 8, 3) == (0, True)


def test_the_sketchs_own_test_case():
    """H16:529-532: Detection{100, 100, 200, 200, 0.9, 0, "person"} at 0.5 m, width 640: CRITICAL, LEFT, all three flags, and
    "person, 0.5 meters" spoken with interrupt, a beep and the critical alert on the left."""
    case = AC.sketch()
    assert case.status == 0 and case.nevents.tolist() == [1]
    e = case.events[0][0]
    assert (e["frame"], e["source"], e["class_id"], e["direction"], e["priority"]) == (0, 3, 0, R.LEFT, R.CRITICAL)
    assert e["distance"] == f32(0.5) and e["flags"] == R.BEEP | R.CRITICAL_ALERT | R.INTERRUPT
    names = ["person", "bicycle", "car"]
    assert R.message(e, names) == "person, 0.5 meters"
    assert R.audio_calls(e, names) == [("speak", "person, 0.5 meters", 3, True), ("playBeep", R.LEFT, 800, 200, f32(0.8)),
                                       ("playCriticalAlert", R.LEFT)]
    far = np.zeros(1, R.EVENT_DTYPE)[0]
    far["class_id"], far["distance"] = -1, 5.0
    assert R.message(far) == "obstacle" and R.audio_calls(far) == [("speak", "obstacle", 0, False)]
    far["distance"] = np.nextafter(f32(5.0), f32(0))
    assert R.message(far) == "obstacle, 5.0 meters"
    assert R.c_fixed1(f32(0.25)) == "0.2" and R.c_fixed1(f32(0.35)) == "0.3" and R.c_fixed1(f32(0.95)) == "0.9"   # 0.35f < 0.35, 0.95f < 0.95


def test_priority_boundaries():
    c = R.config()
    below = lambda v: np.nextafter(f32(v), f32(0))   # noqa: E731
    for cid in (0, 56):                                   # person: dangerous; chair: not
        assert R.priority(c, cid, f32(1.0)) == (R.HIGH if cid == 0 else R.MEDIUM) and R.priority(c, cid, below(1.0)) == R.CRITICAL
        assert R.priority(c, cid, f32(2.0)) == R.MEDIUM and R.priority(c, cid, below(2.0)) == (R.HIGH if cid == 0 else R.MEDIUM)
        assert R.priority(c, cid, f32(3.0)) == R.LOW and R.priority(c, cid, below(3.0)) == R.MEDIUM
    assert R.priority(c, 0, f32(1.5)) == R.HIGH and R.priority(c, 56, f32(1.5)) == R.MEDIUM
    assert R.priority(c, -1, f32(1.5)) == R.HIGH and R.priority(c._replace(obstacle_dangerous=0), -1, f32(1.5)) == R.MEDIUM
    # flags: BEEP strictly below 1.5 m
    m = np.zeros(1, R.MEAS_DTYPE)[0]
    d = np.array(AC.det(300, 0, 340, 9, 0), R.DETECTION_DTYPE)
    for dist, want in ((f32(1.5), 0), (below(1.5), R.BEEP), (below(1.0), R.BEEP | R.CRITICAL_ALERT | R.INTERRUPT)):
        m["distance"], m["flags"] = dist, R.MEAS_SOURCE | R.MEAS_OK
        assert R.classify(c, 3, m, d)[4] == want
    m["flags"] = R.MEAS_SOURCE
    assert R.classify(c, 3, m, d) == (0, R.CENTER, R.LOW, f32(5.0), R.NO_DEPTH)
    # zones: a candidate strictly below zone_alert_m, never without a measurement
    assert R.classify(c, 1, m) is None
    m["distance"], m["flags"] = f32(3.0), R.MEAS_SOURCE | R.MEAS_OK
    assert R.classify(c, 1, m) is None
    m["distance"] = below(3.0)
    assert R.classify(c, 2, m) == (-1, R.RIGHT, R.MEDIUM, below(3.0), 0)


def test_directions_and_keys():
    c = R.config(width=640)
    m = np.zeros(1, R.MEAS_DTYPE)[0]
    dirs = lambda x1, x2: R.classify(c, 3, m, np.array(AC.det(x1, 0, x2, 9, 0), R.DETECTION_DTYPE))[1]   # noqa: E731
    assert dirs(100, 200) == R.LEFT and dirs(270, 370) == R.CENTER and dirs(500, 600) == R.RIGHT
    assert dirs(np.nan, 5) == R.CENTER and dirs(-np.inf, np.inf) == R.CENTER and dirs(0, np.inf) == R.RIGHT and dirs(-np.inf, 0) == R.LEFT
    assert R.key_of(-1, 0) == 0 and R.key_of(0, 2) == 5 and R.key_of(-7, 1) == 4 and R.key_of(83, 2) == 254 == R.key_of(5000, 2)


def test_timeline_of_rule_5():
    case = AC.timeline()
    ev = case.events[0]
    assert case.status == R.E_INVALID                    # frame 7's timestamp decreases
    got = [(int(e["frame"]), int(e["class_id"]), int(e["priority"]), float(e["distance"]), int(e["flags"])) for e in ev]
    crit = R.BEEP | R.CRITICAL_ALERT | R.INTERRUPT
    assert got == [(0, 56, R.MEDIUM, 2.5, 0),            # never announced
                   (2, 56, R.MEDIUM, 2.5, 0),            # frame 1 one nanosecond short; frame 2 exactly at the cooldown
                   (3, 56, R.CRITICAL, f32(0.9), crit),  # escalation inside the cooldown; frame 4's de-escalation is suppressed
                   (5, 62, R.MEDIUM, f32(1.2), R.BEEP), (5, 61, R.MEDIUM, 2.0, 0),       # two of three
                   (6, 70, R.LOW, 5.0, R.NO_DEPTH), (6, 71, R.LOW, 5.0, R.NO_DEPTH),     # the tie falls to the source index
                   (8, 73, R.CRITICAL, 0.5, crit)]       # frame 7 skipped; frame 8 at the last accepted stamp is taken
    assert [int(e["source"]) for e in ev] == [3, 3, 3, 5, 4, 3, 4, 3]
    after = case.states[1][0]
    assert after["events_total"] == 8 and after["reserved"] == 0
    k56 = R.key_of(56, R.CENTER)
    assert after["last_ns"][k56] == 900 * MS and after["last_prio1"][k56] == R.CRITICAL + 1
    assert int((after["last_prio1"] != 0).sum()) == 6     # 56, 62, 61, 70, 71, 73
    # CRITICAL has no cooldown: the same key again one nanosecond later; MEDIUM after it waits out its 800 ms
    c = case.cfg
    spec = [(0, (0.5, None, None), []), (1, (0.5, None, None), []), (2, (2.5, None, None), []), (2000 * MS, (2.5, None, None), [])]
    again = AC.make_arb(c, *AC.build_frames(c, spec), [0, 4], 8)
    assert [int(e["frame"]) for e in again.events[0]] == [0, 1, 3] and again.status == 0


def test_shared_cases_hold_what_the_gpu_tests_lean_on():
    many = AC.many_tracks()
    assert len(many.track_offset) == 34 and many.nevents[0] == 0 and many.nevents.max() > 8 and many.status == 0
    full = AC.full_house()
    per_frame = np.bincount(full.events[0]["frame"], minlength=3).tolist()
    assert per_frame[:2] == [64, 0] and 0 < per_frame[2] < 64          # the third frame repeats the first: cooldowns hold most back
    e0 = full.events[0][:64]
    assert sorted(e0["source"].tolist()) == list(range(64))
    keys = [(-int(e["priority"]), float(e["distance"]), int(e["direction"]), int(e["source"])) for e in e0]
    assert keys == sorted(keys) and len({k[:3] for k in keys}) < 64            # ordered, with ties that the source index settles
    long = AC.long_track()
    assert 10 < long.nevents[0] < 120
    assert AC.long_track(event_cap=3).status == R.E_OUTPUT_TOO_SMALL
    assert AC.long_track(zone_alert_m=1.0, crit_m=0.5).events[0].tobytes() != long.events[0].tobytes()
    mc = AC.measure_case(37, 19, 5)
    assert mc.status == R.E_INVALID and mc.seen == 63
    ok = (mc.meas["flags"] & R.MEAS_OK) != 0
    assert not ok[0, 3] and mc.meas["n_valid"][0, 3] == 1 and not ok[0, 4] and not ok[0, 5]       # min_valid 4: the 1-pixel box has none
    assert AC.measure_case(37, 19, 5, "first").meas[0, 3].tolist() == (1.0, 1, 0, R.MEAS_SOURCE | R.MEAS_OK)    # min_valid 1
    last = AC.measure_case(37, 19, 5, "last").meas
    assert (last["k"][(last["flags"] & R.MEAS_OK) != 0] == last["n_valid"][(last["flags"] & R.MEAS_OK) != 0] - 1).all()
    assert not ok[1].any() and (mc.meas["n_valid"][2, 3], mc.meas["n_valid"][2, 4]) == (3, 4) and not ok[2, 3] and ok[2, 4]
    assert mc.meas["distance"][2, 4] == 3.0               # k = 4 * 1 // 2 = 2 of (1, 2, 3, 4)
    assert mc.meas["distance"][4, 3] == 1.75 and (mc.meas["flags"][9, :64] != 0).all() and (mc.meas["flags"][10, 3:] == 0).all()
    assert np.isfinite(mc.meas["distance"]).all()
