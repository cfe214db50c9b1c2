"""Guided matching through the C++ adapters on the GPU (aria_hip/HipProjectionMatcher.hpp, MapTracker::setLocalMap) and the
driver flag euroc_frontend --track-map FILE2 --local-map K."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HELD, BOOTSTRAP, PNP, FALLBACK, LOCAL = 0, 1, 2, 3, 4
GAP = 4                                                                        # the blank frame of proj_selftest.cpp


def test_cpp_proj_selftest(aria):
    """tests/cpp/proj_selftest.cpp: a generated 3-D scene of 500 points at depths 3 to 12 seen by seven views 0.1 units and 0.3
    degrees apart; the frames are keypoint and descriptor lists (0.3 px of pixel noise, four flipped descriptor bits per view).

    - the adapter's host form matches landmark i to keypoint i and to nothing else;
    - setLocalMap(0) gives the TrackStep sequence and the poses of a tracker that never heard of the mode, bit for bit;
    - with frame 4 blank and the mode off, the frame after it is FALLBACK or HELD: today's break;
    - with setLocalMap(4, 30) that frame is LOCAL, and so is the next. Its position error against the scene's truth is held to
      the largest error of the frames that today's PnP path placed before the gap (frames 2 and 3 of the mode-off run on the
      same sequence): the reference of the check is the existing code.
    Measured on the MI355X when the mode was added, in scene units: worst PnP error before the gap 0.007879, the LOCAL frame
    after the gap 0.004793 (ratio 0.61; 471 correspondences, 351 inliers), the frame after that 0.017309 (ratio 2.20), and
    0.206999 without the mode (the pose still frame 3's, two steps of 0.1 behind). The issue allows a factor 4 for the older,
    farther landmarks; the measured 0.61 is nowhere near it, so the frame after the gap is held to a factor 2 and the factor 4
    is kept for the frame that follows, whose prediction starts from a LOCAL pose."""
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "proj_selftest.cpp")
    exe = os.path.join(ROOT, "build", "proj_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    kv = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    ad = [int(x) for x in kv["adapter"]]
    assert ad[0] == 500 and ad[1] > 400 and ad[2] == ad[1] and ad[3] > 30 and ad[4] == 1
    off = [int(x) for x in kv["off_equal"]]
    assert off[0] == 1 and off[1:] == [BOOTSTRAP] + [PNP] * 5
    broken = [int(x) for x in kv["gap_off"]]
    assert broken[:GAP - 1] == [BOOTSTRAP, PNP, PNP] and broken[GAP - 1] == HELD and broken[GAP] in (FALLBACK, HELD)
    held = [int(x) for x in kv["gap_on"]]
    assert held[0] == BOOTSTRAP and held[GAP - 1] == HELD and held[GAP] == LOCAL and held[GAP + 1] == LOCAL
    er = kv["errors"]
    worst_pnp, err_local, err_next, err_broken = (float(x) for x in er[:4])
    print("worst PnP error before the gap %.6f, LOCAL frame %.6f (ratio %.2f), the next %.6f, without the mode %.6f"
          % (worst_pnp, err_local, err_local / worst_pnp, err_next, err_broken))
    assert er[6] == "1" and worst_pnp > 0
    assert err_local <= 2 * worst_pnp and err_next <= 4 * worst_pnp
    assert int(er[4]) > 300 and int(er[5]) > 0.5 * int(er[4])
    assert err_broken > 0.15                                                   # without the mode the pose is still frame 3's: 0.2 units behind


def test_euroc_frontend_local_map_flag(aria, tmp_path):
    """The driver flag's plumbing, once, on the synthetic image sequence with --pnp-solver p3p: the run ends well, --pose is
    untouched, every step is accounted for in exactly one class, the local line is printed. The sequence is a 2-D shift of a
    flat scene with no true depth, so this shows that the flag reaches the tracker and nothing about accuracy: that is
    test_cpp_proj_selftest's."""
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 6, w=640, h=480)
    exe = os.path.join(PKG, "euroc_frontend")
    t1, t2, tm = (str(tmp_path / n) for n in ("a.txt", "b.txt", "track.txt"))
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", t1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run([exe, str(tmp_path), "1000", "--pose", t2, "--track-map", tm, "--pnp-solver", "p3p", "--local-map", "4",
                          "--local-radius", "20"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(t1, "rb").read() == open(t2, "rb").read()
    n_frames = len(open(t1).read().splitlines())
    w = [l.split() for l in run.stdout.splitlines() if l.startswith("track pnp")][0]
    local = [l.split() for l in run.stdout.splitlines() if l.startswith("track local")]
    assert len(local) == 1 and local[0][4:] == ["the", "last", "4", "pairs,", "radius", "20.0", "px"], run.stdout
    print(" ".join(w), "|", " ".join(local[0]))
    assert int(w[2]) + int(w[4]) + int(w[6]) + int(w[8]) + int(local[0][2]) == n_frames - 1
    assert len(open(tm).read().splitlines()) == n_frames
    bad = subprocess.run([exe, str(tmp_path), "1000", "--pose", t2, "--local-map", "4"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--track-map" in bad.stderr
