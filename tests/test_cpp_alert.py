"""The C++ side of the obstacle alerts on the MI355X: aria_hip/HipObstacleAlerter.hpp wraps the stage and plays its events through
the reference's port IAudioFeedback, and euroc_frontend --alerts writes the events of the --dense depth maps. Both are held to
the restatement (aria_slam_amd/alert_ref.py); without --alerts every other output of the driver is byte-identical."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_cases as AC   # noqa: E402
from test_cpp_stereo import BASELINE, FRAMES, H, NF, T0, W, _frames, _run, _write_tree   # noqa: E402
from aria_slam_amd import alert_ref as R   # noqa: E402

NAMES = ["person", "bicycle", "car"]
PRIO = ["LOW", "MEDIUM", "HIGH", "CRITICAL"]
DIRS = ["CENTER", "LEFT", "RIGHT"]


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


@pytest.fixture(scope="module")
def selftest(built):
    exe = os.path.join(ROOT, "build", "alert_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "alert_selftest.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), src, "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    return exe


def _call_lines(event, names=None):
    """The lines RecordingAudioFeedback keeps for the calls an event makes, from the restatement's audio_calls."""
    out = []
    for c in R.audio_calls(event, names):
        if c[0] == "speak":
            out.append("speak %s %s %s" % (PRIO[c[2]], "interrupt" if c[3] else "-", c[1]))
        elif c[0] == "playBeep":
            out.append("beep %s %d %d %.1f" % (DIRS[c[1]], c[2], c[3], c[4]))
        else:
            out.append("critical %s" % DIRS[c[1]])
    return out


def _sequence():
    """Three frames of 64 x 48. 0: open floor at 4 m and a person (class 0) 0.5 m away on the left: the LEFT zone and the box are
    both CRITICAL. 1: a wall 1.2 m ahead in the centre (HIGH, with a beep) and something at 2.5 m on the right (MEDIUM), which is
    also a box of class 56 ("object" beyond the three names): max_events_per_frame = 2 holds the box back. 2: 100 ms later the
    same frame: the zones are inside their cooldowns, and the box is announced now."""
    Wd, Hd = 64, 48
    f0 = np.full((Hd, Wd), 4.0, np.float32)
    f0[10:40, 4:16] = 0.5
    f1 = np.full((Hd, Wd), 4.0, np.float32)
    f1[12:48, 24:40] = 1.2
    f1[20:40, 50:60] = 2.5
    dets = [[AC.det(4, 10, 16, 40, 0)], [AC.det(50, 20, 60, 40, 56)], [AC.det(50, 20, 60, 40, 56)]]
    ts = [1000 * AC.MS, 1600 * AC.MS, 1700 * AC.MS]
    return Wd, Hd, [f0, f1, f1.copy()], dets, ts


@pytest.mark.parametrize("mode", ["host", "device"])
def test_alerter_plays_the_restatements_events_in_order(selftest, tmp_path, mode):
    Wd, Hd, frames, dets, ts = _sequence()
    cfg = R.config(width=Wd, height=Hd, zone_top=Hd // 4, zone_bottom=Hd, min_valid=4)
    d = np.zeros((3, 1), R.DETECTION_DTYPE)
    for f in range(3):
        d[f, 0] = dets[f][0]
    states = R.new_state(1)
    events, nevents, status, _ = R.run(cfg, np.stack(frames), [0, 3], np.array(ts, np.int64), states, 64, d, np.ones(3, np.int32))
    assert status == 0 and nevents[0] >= 3
    want = []
    for e in events[0]:
        want.append("event %d %d %d %d %d %.9g %d" % (e["frame"], e["source"], e["class_id"], e["direction"], e["priority"], e["distance"], e["flags"]))
        want += _call_lines(e, NAMES)
    n_beeps = int(sum(bool(e["flags"] & R.BEEP) for e in events[0]))
    n_crit = int(sum(bool(e["flags"] & R.CRITICAL_ALERT) for e in events[0]))
    want += ["state %d spoken %d beeps %d critical %d" % (nevents[0], nevents[0], n_beeps, n_crit), "refused"]
    # what the sequence is built to show
    assert want[:8] == ["event 0 1 -1 1 3 0.5 7", "speak CRITICAL interrupt obstacle, 0.5 meters", "beep LEFT 800 200 0.8", "critical LEFT",
                        "event 0 3 0 1 3 0.5 7", "speak CRITICAL interrupt person, 0.5 meters", "beep LEFT 800 200 0.8", "critical LEFT"]
    assert want[8:13] == ["event 1 0 -1 0 2 1.20000005 1", "speak HIGH - obstacle, 1.2 meters", "beep CENTER 800 200 0.8",
                          "event 1 2 -1 2 1 2.5 0", "speak MEDIUM - obstacle, 2.5 meters"]
    assert want[13:15] == ["event 2 3 56 2 1 2.5 0", "speak MEDIUM - object, 2.5 meters"] and len(want) == 17
    path = str(tmp_path / "in.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", Wd, Hd, 3, len(NAMES)))
        for n in NAMES:
            f.write(n.encode().ljust(16, b"\0"))
        for i in range(3):
            f.write(struct.pack("<qi", ts[i], 1))
            f.write(d[i].tobytes())
            f.write(frames[i].tobytes())
    got = _run(selftest, mode, path).splitlines()
    print("\n".join(got))
    assert got == want


def test_euroc_frontend_alerts_equal_the_restatement(aria, built, tmp_path):
    """Zones over the dense depth maps of the four stereo frames (this driver sets no detector): the lines of --alerts are the
    restatement's events with the calls each made, and every other output is byte-identical without the flag."""
    from aria_slam_amd import dense_ref as DR
    frames = _frames()
    root = str(tmp_path / "seq")
    _write_tree(root, frames)
    names = ("stereo.txt", "pose.txt", "frames.csv", "dense.txt")
    with_flag = {k: str(tmp_path / ("a_" + k)) for k in names}
    without = {k: str(tmp_path / ("p_" + k)) for k in names}
    common = lambda f: ["--stereo", BASELINE, "--stereo-out", f["stereo.txt"], "--pose", f["pose.txt"], "--csv", f["frames.csv"],   # noqa: E731
                        "--dense", f["dense.txt"]]
    out_file = str(tmp_path / "alerts.txt")
    stdout = _run(built, root, NF, *common(with_flag), "--alerts", out_file)
    depth = np.stack([DR.depth_map(DR.dense_disparity(l, r), DR.EUROC_K, BASELINE) for l, r in frames]).astype(np.float32)
    ts = np.array([int(round(float(str(T0 + f * 50_000_000)) * 1e-9 * 1e9)) for f in range(FRAMES)], np.int64)
    cfg = R.config(width=W, height=H, zone_top=H // 4, zone_bottom=H)
    events, nevents, status, meas = R.run(cfg, depth, [0, FRAMES], ts, R.new_state(1), 64)
    print(meas[:, :3], nevents)
    want = []
    for e in events[0]:
        want.append("%d %d %d %d %d %d %.9g %d | %s" % (ts[e["frame"]], e["frame"], e["source"], e["class_id"], e["direction"], e["priority"],
                                                          e["distance"], e["flags"], "; ".join(_call_lines(e))))
    got = open(out_file).read().splitlines()
    assert got == want and status == 0
    assert len(got) >= 1                                            # the scene is closer than zone_alert_m somewhere
    line = [l for l in stdout.splitlines() if l.startswith("alerts")]
    assert line == ["alerts %d %d" % (len(want), FRAMES)]
    stdout2 = _run(built, root, NF, *common(without))
    assert not any(l.startswith("alerts") for l in stdout2.splitlines())
    for k in names:
        assert open(with_flag[k], "rb").read() == open(without[k], "rb").read(), k
    refused = subprocess.run([built, root, str(NF), "--alerts", out_file], capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--alerts needs" in refused.stderr


def test_adapters_library_holds_the_alerter_classes(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipObstacleAlerter::process", "aria::adapters::hip::HipObstacleAlerter::processDevice",
                 "aria::adapters::hip::HipObstacleAlerter::message", "aria::adapters::hip::RecordingAudioFeedback::speak",
                 "aria::adapters::hip::RecordingAudioFeedback::playBeep", "aria::factory::createHipAlerter"):
        assert name in syms, name
