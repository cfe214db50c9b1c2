"""The C++ side of frame-to-model tracking (aria_slam_amd/host: HipDenseTracker, DenseTracker): tests/cpp/icp_selftest.cpp builds
against the adapters and, on the GPU, tracks six frames of a generated 3-D scene with DenseTracker; euroc_frontend
--track-dense runs the same loop on the sequence the other test_cpp_* files build."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
EXE = os.path.join(ROOT, "build", "icp_selftest")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _build():
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), os.path.join(ROOT, "tests", "cpp", "icp_selftest.cpp"), "-o", EXE,
                           "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])


def test_icp_selftest_builds_against_the_adapters(aria):
    _build()
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True, check=True).stdout
    for m in ("HipDenseTracker::track", "HipDenseTracker::trackBatchDevice", "HipDenseTracker::requireSameIntrinsics",
              "DenseTrackerConfig::fromRenderer", "DenseTracker::step"):
        assert "aria::adapters::hip::" + m in syms, m


@pytest.mark.gpu
def test_cpp_icp_selftest(aria):
    """Frame 0 has no model and is integrated where it is; frames 1-5 are tracked against the cast volume with the previous
    estimate as the guess, so each starts a whole step (0.02 rad, 0.032 m) away. Every one is valid with thousands of
    correspondences and ends nearer the truth than its prediction was. A tracker that did nothing would end 0.1 rad and 0.158 m
    off: the bound is half of that, which leaves the fused model's own bias (about a centimetre, tests/icp_cases.py) five
    steps of room. A configuration the stage refuses throws."""
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    rows = [l.split() for l in out.stdout.splitlines() if l.strip()]
    frames = [r for r in rows if r[0] == "frame"]
    assert len(frames) == 6 and frames[0][2:5] == ["0", "0", "0"]
    for r in frames[1:]:
        assert r[2:5] == ["1", "0", "1"] and int(r[5]) > 2000, r
        assert float(r[8]) < float(r[9]), r                          # nearer than the prediction
    final = [r for r in rows if r[0] == "final"][0]
    assert float(final[1]) < 0.5 * float(final[3]) and float(final[2]) < 0.5 * float(final[4]) and final[5] == "0"
    assert [r for r in rows if r[0] == "refused"][0][1] == "1"


@pytest.mark.gpu
def test_euroc_frontend_track_dense_writes_a_trajectory_and_changes_nothing_else(aria, tmp_path):
    """The sequence the other test_cpp_* files build (a window sliding over one synthetic pair: a flat scene). The flag is
    exercised for plumbing, as --track-map and --bundle are: one TUM line per frame with finite fields, one summary line with
    lost <= tracked and at least one tracked frame, the lost count on stderr, a "track-dense" line in the --eval file when the
    sequence has ground truth or none of it when not, and every other output byte-identical without the flag."""
    from test_cpp_stereo import BASELINE, NF, _frames, _run, _write_tree
    _build()
    exe = os.path.join(PKG, "euroc_frontend")
    root = str(tmp_path / "seq")
    frames = _frames()
    _write_tree(root, frames)
    names = ("stereo.txt", "pose.txt", "frames.csv", "dense.txt", "volume.ply")

    def common(f):
        return ["--stereo", BASELINE, "--stereo-out", f["stereo.txt"], "--pose", f["pose.txt"], "--csv", f["frames.csv"],
                "--dense", f["dense.txt"], "--volume", f["volume.ply"], "--voxel", 0.1]
    with_flag = {k: str(tmp_path / ("w_" + k)) for k in names}
    tum = str(tmp_path / "dense_track.txt")
    stdout = _run(exe, root, NF, *common(with_flag), "--track-dense", tum)
    line = [l for l in stdout.splitlines() if l.startswith("track-dense")]
    assert len(line) == 1 and line[0].split()[1] == "tracked" and line[0].split()[3] == "lost", line
    tracked, lost = int(line[0].split()[2]), int(line[0].split()[4])
    print(line[0])
    assert 1 <= tracked <= len(frames) - 1 and 0 <= lost <= tracked
    rows = [l.split() for l in open(tum).read().splitlines()]
    assert len(rows) == len(frames) and all(len(r) == 8 for r in rows)
    import math
    assert all(math.isfinite(float(x)) for r in rows for x in r)
    assert all(abs(sum(float(x) ** 2 for x in r[4:]) - 1.0) < 1e-6 for r in rows)                 # unit quaternions
    without = {k: str(tmp_path / ("p_" + k)) for k in names}
    stdout = _run(exe, root, NF, *common(without))
    assert not any(l.startswith("track-dense") for l in stdout.splitlines())
    for k in names:
        assert open(with_flag[k], "rb").read() == open(without[k], "rb").read(), k
    refused = subprocess.run([exe, root, str(NF), "--track-dense", tum], capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--track-dense needs" in refused.stderr
