"""The C++ side of the bundle-adjustment stage (aria_slam_amd/host: HipBundleAdjuster, WindowBuilder, MapTracker's hook):
tests/cpp/ba_selftest.cpp builds against the adapters and, on the GPU, tracks a six-frame synthetic 3-D scene with MapTracker,
builds windows from what the tracker did and adjusts them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
EXE = os.path.join(ROOT, "build", "ba_selftest")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), os.path.join(ROOT, "tests", "cpp", "ba_selftest.cpp"), "-o", EXE,
                           "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])


def test_ba_selftest_builds_against_the_adapters(aria):
    _build()
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True, check=True).stdout
    for m in ("HipBundleAdjuster::optimize", "HipBundleAdjuster::optimizeBatchDevice", "WindowBuilder::addStep", "WindowBuilder::window",
              "WindowBuilder::store"):
        assert "aria::adapters::hip::" + m in syms, m


@pytest.mark.gpu
def test_cpp_ba_selftest(aria):
    """MapTracker bootstraps the first pair and places the other four frames by PnP; the builder holds six frames and the
    tracks of every step (a quarter of them end at step 3, whose match list is cut). The six-frame window -- sorted
    observations, tracks of two to six views -- is adjusted with two poses fixed: valid, chi2 falls, the residual ends near the
    pixel noise (0.3 px per axis: 0.42 px rms; the bound is 1 px), the fixed poses keep their bits. Two sliding windows of four
    frames: the first's refined poses seed the second. An invalid window throws."""
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    rows = [l.split() for l in out.stdout.splitlines() if l.strip()]
    steps = [r for r in rows if r[0] == "step"]
    assert len(steps) == 5 and steps[0][2] == "1" and all(s[2] == "2" for s in steps[1:]), steps     # BOOTSTRAP, then PNP
    assert all(int(s[4]) > 200 for s in steps)
    kv = {r[0]: r[1:] for r in rows if r[0] != "step"}
    assert int(kv["builder"][0]) == 6 and int(kv["builder"][1]) == sum(int(s[4]) for s in steps) and int(kv["builder"][2]) == 4
    n_poses, n_points, n_obs, full, two, is_sorted = (int(x) for x in kv["window"])
    assert n_poses == 6 and n_points == int(kv["builder"][1]) and full > 100 and two > 100 and is_sorted == 1
    assert 2 * n_points < n_obs <= 6 * n_points
    adj = kv["adjust"]
    valid, stop, chi0, chi1, rms, its, used = int(adj[0]), int(adj[1]), float(adj[2]), float(adj[3]), float(adj[4]), int(adj[5]), int(adj[6])
    assert valid == 1 and stop in (0, 1) and its >= 1 and chi1 < chi0 and rms < 1.0 and used == n_obs
    assert int(adj[9]) == 1                                          # the fixed poses keep their bits
    sl = kv["slide"]
    assert sl[0] == sl[1] == "1" and float(sl[3]) < float(sl[2]) and float(sl[5]) <= float(sl[4]) and sl[8] == "1"
    assert int(sl[6]) > 0 and int(sl[7]) > 0
    assert kv["invalid"] == ["1"]


@pytest.mark.gpu
def test_euroc_frontend_bundle(aria, tmp_path):
    """The driver flag on the synthetic image sequence, for its plumbing: the scene is a 2-D shift of a flat scene, which gives
    PnP nothing to place (test_gpu_pnp.py), so what bundle adjustment does on a 3-D scene is test_cpp_ba_selftest's. One TUM
    line per frame and one comment line per window; --track-map's own output is untouched; no window ends above where it
    began."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 6, w=640, h=480)          # 6 synthetic pairs: 12 frames
    exe = os.path.join(PKG, "euroc_frontend")
    p1, p2, t1, t2, bf = (str(tmp_path / n) for n in ("p1.txt", "p2.txt", "t1.txt", "t2.txt", "bundle.txt"))
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", p1, "--track-map", t1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run([exe, str(tmp_path), "1000", "--pose", p2, "--track-map", t2, "--bundle", bf, "--bundle-window", "5"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(t1, "rb").read() == open(t2, "rb").read() and open(p1, "rb").read() == open(p2, "rb").read()
    print([l for l in run.stdout.splitlines() if l.startswith(("bundle", "track "))])
    lines = open(bf).read().splitlines()
    rows = [l.split() for l in lines if not l.startswith("#")]
    windows = [l.split() for l in lines if l.startswith("# window")]
    assert len(rows) == 12 and all(len(r) == 8 and all(np.isfinite(float(x)) for x in r) for r in rows)
    assert [float(x) for x in rows[0][1:]] == [0, 0, 0, 0, 0, 0, 1]          # a window's first two poses are fixed
    assert [w[2] for w in windows] == ["0", "3", "6", "9"] and [w[3] for w in windows] == ["5", "5", "5", "3"]   # stride N - 2
    for w in windows:
        kv = dict(zip(w[4::2], w[5::2]))
        print(" ".join(w))
        c0, c1, rms = float(kv["chi2_initial"]), float(kv["chi2_final"]), float(kv["rms_px"])
        assert np.isfinite([c0, c1, rms]).all() and c1 <= c0
    assert lines[-len(windows):] == [l for l in lines if l.startswith("#")]     # the comment lines trail the poses
    bad = subprocess.run([exe, str(tmp_path), "1000", "--pose", p1, "--bundle", bf], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--track-map" in bad.stderr
