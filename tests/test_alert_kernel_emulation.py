"""The plain device functions of aria_slam_amd/csrc/alert_stage.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/alert_ref.py) on the cases tests/test_gpu_alert.py runs on the device.

The text of the file between "// ---- rules" and "// ---- kernels" -- rule 1 (zones, detection counts and rectangles), the
valid-depth test and the rank of rule 2, rule 3's classification, rule 4's comparison and rule 5's key and test -- is pasted
between tests/cpp/alert_rules_emu_head.inc (a shim: the qualifiers defined away) and alert_rules_emu_tail.inc (the parameters,
and the arbitration kernel's use of those functions restated with the 64 lanes of a wave one after the other) and compiled with
the clang++ that hipcc drives. What this checks without a GPU is every rule's arithmetic and the order in which the walk applies
them. What it cannot check stays on the GPU (tests/test_gpu_alert.py): the histogram kernel -- its walk of a rectangle, the LDS
atomics, the workgroup scan and the narrowing over three passes -- and the wave ranking of the arbitration kernel through
ballots and shuffles, the device's streams and the lifecycle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_cases as AC   # noqa: E402
from aria_slam_amd import alert_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "alert_stage.hip")).read()
    body = src[src.index("\n// ---- rules"):src.index("\n// ---- kernels")]
    for k in ("alert_direction", "alert_column_zone", "alert_det_count", "alert_source_rect", "alert_valid_depth", "alert_rank",
              "alert_priority", "alert_classify", "alert_precedes", "alert_key", "alert_may_announce"):
        assert k in body, k
    for word in ("asm", "__shared__", "__syncthreads", "__shfl", "__ballot", "atomic"):
        assert word not in body, "plain functions, no cross-lane operation: " + word
    head, tail = (open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("alert_rules_emu_head.inc", "alert_rules_emu_tail.inc"))
    out_dir = os.path.join(ROOT, "build", "alert_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "alert_emu.cpp"), os.path.join(out_dir, "libalert_emu.so")
    with open(cpp, "w") as f:
        f.write(head + body + tail)
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I", os.path.join(ROOT, "include"),
                           "-o", so, cpp])
    L = C.CDLL(so)
    p, i = C.c_void_p, C.c_int
    L.emu_column_zone.argtypes = [i, i]
    L.emu_rank.restype = C.c_longlong
    L.emu_rank.argtypes = [C.c_longlong, i, i]
    L.emu_valid.argtypes = [p, p, p, C.c_float]
    L.emu_sources.argtypes = [p, p, p, p, i, i, p, p, p]
    L.emu_arbitrate.argtypes = [p, p, p, p, i, p, i, p, p, p, i, p, p, i, p]
    return L


def _params(c):
    b0, b1 = R.zone_bounds(c.width)
    ip = np.array([c.width, c.height, c.zone_top, c.zone_bottom, b0, b1, c.max_dets, c.min_valid, *c.zone_pct, *c.det_pct,
                   c.obstacle_dangerous, len(c.dangerous), c.max_events_per_frame, *c.dangerous, *([0] * (32 - len(c.dangerous)))], np.int32)
    fp = np.array([c.min_depth, c.max_depth, c.zone_alert_m, c.default_depth, c.crit_m, c.high_m, c.medium_m, c.beep_m], np.float32)
    lp = np.array(c.cooldown_ns, np.int64)
    return ip, fp, lp


@pytest.mark.parametrize("width", [1, 3, 20, 37, 640, 752])
def test_column_zone(emu, width):
    assert [emu.emu_column_zone(x, width) for x in range(width)] == [R.column_zone(x, width) for x in range(width)]


def test_rank_and_valid_depth(emu):
    for n in (0, 1, 4, 99, 100, 94680, 2 ** 26):
        for num, den in ((5, 100), (1, 2), (0, 1), (1048575, 1048576), (2147483646, 2147483647)):
            assert emu.emu_rank(n, num, den) == n * num // den
    c = R.config()
    ip, fp, lp = _params(c)
    f32 = np.float32
    vals = [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-40, 0.1, np.nextafter(f32(0.1), f32(0)), 20.0, np.nextafter(f32(20), f32(30)), 3.0]
    got = [emu.emu_valid(ip.ctypes.data, fp.ctypes.data, lp.ctypes.data, float(f32(v))) for v in vals]
    assert got == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("W,H", AC.SIZES)
def test_sources_of_every_measure_frame(emu, W, H):
    """Rule 1 on the frames of the measurement cases: which slots are sources, their rectangles, the deferred error and the
    largest count above max_dets."""
    case = AC.measure_case(W, H, 0)
    ip, fp, lp = _params(case.cfg)
    err, seen = 0, np.zeros(1, np.int32)
    for f in range(len(case.ndets)):
        rects, used = np.full((64, 4), -7, np.int32), np.full(64, -7, np.int32)
        d = np.ascontiguousarray(case.dets[f])
        err |= emu.emu_sources(ip.ctypes.data, fp.ctypes.data, lp.ctypes.data, d.ctypes.data, int(case.ndets[f]), AC.DET_CAP,
                               rects.ctypes.data, used.ctypes.data, seen.ctypes.data)
        n_det, _ = R.det_count(int(case.ndets[f]), AC.DET_CAP, case.cfg.max_dets)
        for s in range(64):
            if s >= 3 + n_det:
                assert used[s] == 0 and case.meas["flags"][f, s] == 0
                continue
            x0, y0, x1, y1 = R.source_rect(case.cfg, s, case.dets[f, s - 3] if s >= 3 else None)
            empty = x0 >= x1 or y0 >= y1
            assert used[s] == (2 if empty else 1), (f, s)
            if not empty:
                assert rects[s].tolist() == [x0, y0, x1, y1], (f, s)
                assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H       # what the kernel reads lies inside the map
    assert err == 1 and seen[0] == 63 == case.seen


def _arbitrate(emu, case):
    ip, fp, lp = _params(case.cfg)
    n_tracks = len(case.track_offset) - 1
    states = case.states[0].copy()
    events = np.full((n_tracks, case.event_cap + 1), AC.GUARD, np.uint8).repeat(32, axis=1).view(R.EVENT_DTYPE)
    events = np.ascontiguousarray(events.reshape(-1)[:n_tracks * case.event_cap + 1])
    nev = np.full(n_tracks + 1, -7, np.int32)
    a = [np.ascontiguousarray(x) for x in (case.track_offset, case.timestamps, case.meas, case.dets, case.ndets)]
    err = emu.emu_arbitrate(ip.ctypes.data, fp.ctypes.data, lp.ctypes.data, a[0].ctypes.data, n_tracks, a[1].ctypes.data, len(case.timestamps),
                            a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data, case.dets.shape[1], states.ctypes.data, events.ctypes.data,
                            case.event_cap, nev.ctypes.data)
    assert err >= 0, "rule 4 gave two candidates one rank"
    assert nev[-1] == -7 and (events[-1:].view(np.uint8) == AC.GUARD).all()
    return events[:-1].reshape(n_tracks, case.event_cap), nev[:-1], states, err


@pytest.mark.parametrize("name", ["timeline", "sketch", "full_house", "many_tracks", "long_track", "long_track_cap3", "long_track_strict"])
def test_arbitration_cases_are_bitwise_the_restatement(emu, name):
    case = {"long_track_cap3": lambda: AC.long_track(event_cap=3), "long_track_strict": lambda: AC.long_track(zone_alert_m=1.0, crit_m=0.5)}.get(
        name, getattr(AC, name, None))()
    ev, nev, states, err = _arbitrate(emu, case)
    assert nev.tobytes() == case.nevents.tobytes()
    for t, want in enumerate(case.events):
        n = min(len(want), case.event_cap)
        assert ev[t, :n].tobytes() == want[:n].tobytes(), (name, t)
        assert (ev[t, n:].view(np.uint8) == AC.GUARD).all()
    assert states.tobytes() == case.states[1].tobytes()
    assert {0: 0, 1: R.E_INVALID, 2: R.E_OUTPUT_TOO_SMALL, 3: R.E_INVALID}[err] == case.status
