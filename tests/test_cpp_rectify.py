"""The C++ side of rectification on the MI355X: AslSequence reads mav0/cam0/sensor.yaml and mav0/cam1/sensor.yaml,
aria_hip/HipRectifier.hpp wraps the stage and equals the Python binding, and euroc_frontend --rectify --stereo prints per
frame what the Python chain computes from the same raw images. Without --rectify the driver's outputs do not change, with
or without the sensor.yaml files in the tree."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as RC   # noqa: E402

W, H, NF, FRAMES = 320, 240, 500, 4
T0 = 1403636579763555584


def _calibration():
    from aria_slam_amd import rectify_ref as R
    return R.scaled_calibration(W, H, RC.EUROC)


def _raw_frames():
    """Four raw pairs: a 328-px-wide rectified stereo_scene pair seen through a window that moves 2 px per frame, each
    window inverse-warped into the two distorted, rotated cameras."""
    from aria_slam_amd import rectify_ref as R
    from aria_slam_amd import stereo_ref as S
    left, right, _ = S.stereo_pair(11, W + 2 * FRAMES, H)
    cal = _calibration()
    return [R.raw_from_rectified(left[:, 2 * f:2 * f + W], right[:, 2 * f:2 * f + W], cal) for f in range(FRAMES)]


def _write_tree(root, frames, cal, yaml=(True, True), size=(W, H)):
    from test_frontend_io import write_png
    for cam, side in (("cam0", 0), ("cam1", 1)):
        d = os.path.join(root, "mav0", cam, "data")
        os.makedirs(d, exist_ok=True)
        rows = []
        for f, pair in enumerate(frames):
            ts = T0 + f * 50_000_000
            open(os.path.join(d, "%d.png" % ts), "wb").write(write_png(pair[side]))
            rows.append("%d,%d.png" % (ts, ts))
        with open(os.path.join(root, "mav0", cam, "data.csv"), "w") as fh:
            fh.write("#timestamp [ns],filename\n" + "\n".join(rows) + "\n")
        if yaml[side]:
            RC.write_sensor_yaml(os.path.join(root, "mav0", cam, "sensor.yaml"), cal["K_l" if side == 0 else "K_r"],
                                 cal["D_l" if side == 0 else "D_r"], cal["T_BS_l" if side == 0 else "T_BS_r"], size)


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


@pytest.fixture(scope="module")
def selftest(built):
    exe = os.path.join(ROOT, "build", "rect_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "rect_selftest.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), src, "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _fnv(b):
    h = 1469598103934665603
    for v in b:
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_adapter_and_reader_equal_the_python_binding(aria, selftest, tmp_path):
    """Shape (b) through aria_hip/HipRectifier.hpp: the calibration as AslSequence parsed it from the two sensor.yaml files, the
    geometry, both maps, the five noise frames of both cameras and shape (d)'s full frame of keypoints."""
    root = str(tmp_path / "seq")
    full = dict(RC.EUROC)
    blank = [(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))]
    _write_tree(root, blank, full, size=RC.SIZE)
    frames, kp = RC.noise_frames(), RC.keypoints()[0][2]
    paths = [str(tmp_path / n) for n in ("frames.bin", "out.bin", "kp.bin", "kp_out.bin")]
    frames.tofile(paths[0])
    kp.tofile(paths[2])
    stdout = _run(selftest, root, *paths, RC.N_FRAMES, RC.SMALL[0], RC.SMALL[1], *["%.17g" % v for v in RC.SMALL_NEW_K], RC.FILL)
    lines = stdout.splitlines()
    assert lines[-1] == "DONE"
    for cam, (K, D, T) in enumerate(((RC.K_L, RC.D_L, RC.T_BS_L), (RC.K_R, RC.D_R, RC.T_BS_R))):
        got = [float(v) for v in lines[cam].split()[2:]]
        assert lines[cam].startswith("cal %d " % cam) and got == list(K) + list(D) + [0.0] + list(T) + [752.0, 480.0]
    r = aria.HipRectifier.from_stereo_calibration(RC.K_L, RC.D_L, RC.T_BS_L, RC.K_R, RC.D_R, RC.T_BS_R, RC.SIZE, RC.SMALL,
                                                  RC.SMALL_NEW_K, fill=RC.FILL)
    try:
        assert float(lines[2].split()[1]) == r.baseline
        assert tuple(float(v) for v in lines[3].split()[1:]) == r.new_K
        for cam in range(2):
            assert int(lines[4 + cam].split()[2]) == _fnv(r.map(cam).tobytes())
        out = np.fromfile(paths[1], np.uint8).reshape(2, RC.N_FRAMES, RC.SMALL[1], RC.SMALL[0])
        assert out.tobytes() == RC.ref_remapped().tobytes()
        assert out[1, 3].tobytes() == r.remap(frames[1, 3], 1).tobytes()
        kp_out = np.fromfile(paths[3], kp.dtype).reshape(2, -1)
        for cam in range(2):
            assert kp_out[cam].tobytes() == r.points(kp, cam).tobytes()
    finally:
        r.close()


def _python_lines(aria, frames, cal):
    """What euroc_frontend --rectify --stereo 0 computes, through the Python bindings."""
    r = aria.HipRectifier.from_stereo_calibration(cal["K_l"], cal["D_l"], cal["T_BS_l"], cal["K_r"], cal["D_r"], cal["T_BS_r"], (W, H))
    ext = aria.OrbHipExtractor(max_features=NF, max_width=W, max_height=H)
    st = aria.HipStereoMatcher(K=r.new_K, baseline=r.baseline)
    lines = []
    try:
        for f, (raw_l, raw_r) in enumerate(frames):
            left, right = r.remap(raw_l, 0), r.remap(raw_r, 1)
            obs, m = st.match(left, right, ext.extract(left), ext.extract(right))
            depth = np.sort(obs["depth"][obs["right_idx"] >= 0])
            lines.append("%.9f %d %.9f" % ((T0 + f * 50_000_000) * 1e-9, len(m), float(depth[len(depth) // 2]) if len(depth) else 0.0))
        return lines, r.baseline
    finally:
        for h in (st, ext, r):
            h.close()


def test_euroc_frontend_rectify_stereo_lines_equal_the_python_chain(aria, built, tmp_path):
    frames, cal = _raw_frames(), _calibration()
    root = str(tmp_path / "seq")
    _write_tree(root, frames, cal)
    out = str(tmp_path / "stereo.txt")
    stdout = _run(built, root, NF, "--rectify", "--stereo", 0, "--stereo-out", out)
    want, baseline = _python_lines(aria, frames, cal)
    assert "stereo baseline %.6g m" % baseline in stdout
    got = open(out).read().splitlines()
    assert got == want
    assert all(int(l.split()[1]) > 100 and float(l.split()[2]) > 0 for l in got)
    # the raw pairs without --rectify match far fewer keypoints: what the flag is for
    plain = str(tmp_path / "plain.txt")
    _run(built, root, NF, "--stereo", 0.11, "--stereo-out", plain)
    assert sum(int(l.split()[1]) for l in open(plain)) < 0.5 * sum(int(l.split()[1]) for l in got)
    # cam0 alone: undistortion before extraction, the pose stage on the new K
    pose = str(tmp_path / "pose.txt")
    stdout = _run(built, root, NF, "--rectify", "--pose", pose)
    assert len(open(pose).read().splitlines()) == FRAMES
    # a missing sensor.yaml is a message and an exit status, not a crash
    no_cam1 = str(tmp_path / "no_cam1")
    _write_tree(no_cam1, frames, cal, yaml=(True, False))
    refused = subprocess.run([built, no_cam1, str(NF), "--rectify", "--stereo", "0"], capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1 and "cam1/sensor.yaml" in refused.stderr
    assert subprocess.run([built, no_cam1, str(NF), "--rectify"], capture_output=True, text=True, timeout=300).returncode == 0
    for bad in (["--stereo", "0"], ["--rectify", "--batch", "2"]):
        assert subprocess.run([built, root, str(NF)] + bad, capture_output=True, text=True, timeout=300).returncode != 0


def test_outputs_without_rectify_do_not_change(aria, built, tmp_path):
    """The same frames with and without the sensor.yaml files: --pose, --csv and --stereo-out are byte-identical, equal the
    files the parent commit's build wrote for the same command (tests/golden/rectify_parent/), and the stereo columns are
    what the Python bindings compute with the pinhole defaults."""
    frames, cal = _raw_frames(), _calibration()
    with_yaml, without = str(tmp_path / "a"), str(tmp_path / "b")
    _write_tree(with_yaml, frames, cal)
    _write_tree(without, frames, cal, yaml=(False, False))
    files = {}
    for tag, root in (("a", with_yaml), ("b", without)):
        files[tag] = [str(tmp_path / (tag + n)) for n in ("_pose.txt", ".csv", "_stereo.txt")]
        _run(built, root, NF, "--pose", files[tag][0], "--csv", files[tag][1], "--stereo", 0.25, "--stereo-out", files[tag][2])
    golden = os.path.join(ROOT, "tests", "golden", "rectify_parent")
    for k, name in enumerate(("pose.txt", "frames.csv", "stereo.txt")):
        assert open(files["a"][k], "rb").read() == open(files["b"][k], "rb").read(), k
        # what the commit before --rectify existed wrote for this command on this sequence (its build, on an MI355X)
        assert open(files["a"][k], "rb").read() == open(os.path.join(golden, name), "rb").read(), name
    # the parent's output on this sequence, recomputed: the stereo columns through the bindings with the default K
    ext = aria.OrbHipExtractor(max_features=NF, max_width=W, max_height=H)
    st = aria.HipStereoMatcher(baseline=0.25)
    try:
        for f, (left, right) in enumerate(frames):
            obs, m = st.match(left, right, ext.extract(left), ext.extract(right))
            depth = np.sort(obs["depth"][obs["right_idx"] >= 0])
            want = "%.9f %d %.9f" % ((T0 + f * 50_000_000) * 1e-9, len(m), float(depth[len(depth) // 2]) if len(depth) else 0.0)
            assert open(files["a"][2]).read().splitlines()[f].startswith(want)
    finally:
        st.close()
        ext.close()
    refused = subprocess.run([built, without, str(NF), "--rectify"], capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1 and "sensor.yaml" in refused.stderr
