"""The C++ side of the fisheye (KB4) model on the MI355X: AslSequence reads an `equidistant` sensor.yaml and maps the name to
the model, aria_hip/HipRectifier.hpp with model = KB4 equals the Python binding, euroc_frontend --rectify --stereo 0 runs on
a fisheye rig and prints what the Python chain computes, and a rig of one radtan and one equidistant camera is refused by
name."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisheye_cases as F   # noqa: E402
import rectify_cases as RC   # noqa: E402

W, H, NF, FRAMES = 320, 240, 500, 3
T0 = 1403636579763555584


def _calibration():
    """The rig of fisheye_cases at 320x240."""
    from aria_slam_amd import rectify_ref as R
    return R.scaled_calibration(W, H, F.RIG)


@pytest.fixture(scope="module")
def raw_frames():
    """Three raw fisheye pairs: a rectified stereo_scene pair seen through a window that moves 2 px per frame, each window
    inverse-warped into the two fisheye cameras."""
    from aria_slam_amd import rectify_ref as R
    from aria_slam_amd import stereo_ref as S
    left, right, _ = S.stereo_pair(11, W + 2 * FRAMES, H)
    cal = _calibration()
    return [R.raw_from_rectified(left[:, 2 * f:2 * f + W], right[:, 2 * f:2 * f + W], cal) for f in range(FRAMES)]


def _write_tree(root, frames, cal, models=("equidistant", "equidistant"), size=(W, H)):
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
        F.write_sensor_yaml(os.path.join(root, "mav0", cam, "sensor.yaml"), cal["K_l" if side == 0 else "K_r"],
                            cal["D_l" if side == 0 else "D_r"], cal["T_BS_l" if side == 0 else "T_BS_r"], size, models[side])


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


@pytest.fixture(scope="module")
def selftest(built):
    exe = os.path.join(ROOT, "build", "rect_kb4_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "rect_kb4_selftest.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host", "include"), src, "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                           "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_adapter_and_reader_equal_the_python_binding(aria, selftest, tmp_path):
    """zoom10 through aria_hip/HipRectifier.hpp: the calibration and the model as AslSequence parsed them from an `equidistant`
    sensor.yaml, the map words and a full frame of keypoints."""
    case = F.CASES["zoom10"]
    root = str(tmp_path / "seq")
    blank = [(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))]
    cal = dict(K_l=F.K_A, K_r=F.K_A, D_l=F.D_A, D_r=F.D_A, T_BS_l=RC.T_BS_L, T_BS_r=RC.T_BS_R)
    _write_tree(root, blank, cal, size=F.SRC)
    kp = F.keypoints()[1]
    paths = [str(tmp_path / n) for n in ("map.bin", "kp.bin", "kp_out.bin")]
    kp.tofile(paths[1])
    lines = _run(selftest, root, *paths, case.dst[0], case.dst[1], *["%.17g" % v for v in case.new_K]).splitlines()
    assert lines[-1] == "DONE" and lines[1] == "model equidistant 1"
    assert [float(v) for v in lines[0].split()[1:]] == list(F.K_A) + list(F.D_A) + [0.0] + list(RC.T_BS_L) + [96.0, 64.0]
    r = aria.HipRectifier(cameras=case.cam, new_K=case.new_K, src_size=case.src, dst_size=case.dst)
    try:
        got = np.fromfile(paths[0], np.uint32).reshape(case.dst[1], case.dst[0])
        assert got.tobytes() == r.map(0).tobytes() == case.map.tobytes()
        assert np.fromfile(paths[2], kp.dtype).tobytes() == r.points(kp).tobytes()
    finally:
        r.close()


def _python_lines(aria, frames, cal):
    """What euroc_frontend --rectify --stereo 0 computes, through the Python bindings."""
    r = aria.HipRectifier.from_stereo_calibration(cal["K_l"], cal["D_l"], cal["T_BS_l"], cal["K_r"], cal["D_r"], cal["T_BS_r"], (W, H),
                                                  model="kb4")
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


def test_euroc_frontend_rectifies_a_fisheye_rig(aria, built, raw_frames, tmp_path):
    cal = _calibration()
    root = str(tmp_path / "seq")
    _write_tree(root, raw_frames, cal)
    out = str(tmp_path / "stereo.txt")
    stdout = _run(built, root, NF, "--rectify", "--stereo", 0, "--stereo-out", out)
    want, baseline = _python_lines(aria, raw_frames, cal)
    assert "stereo baseline %.6g m" % baseline in stdout
    got = open(out).read().splitlines()
    assert len(got) == FRAMES and got == want
    assert all(int(l.split()[1]) > 20 and float(l.split()[2]) > 0 for l in got)
    for name in ("fisheye", "kb4"):                                                  # the other two names of the model
        other = str(tmp_path / name)
        _write_tree(other, raw_frames[:1], cal, models=(name, name))
        _run(built, other, NF, "--rectify", "--stereo", 0, "--stereo-out", out)
        assert open(out).read().splitlines() == want[:1]


def test_euroc_frontend_refuses_a_rig_of_two_models(built, raw_frames, tmp_path):
    cal = _calibration()
    root = str(tmp_path / "mixed")
    _write_tree(root, raw_frames[:1], cal, models=("radial-tangential", "equidistant"))
    refused = subprocess.run([built, root, str(NF), "--rectify", "--stereo", "0"], capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1
    assert "radial-tangential" in refused.stderr and "equidistant" in refused.stderr and "differ" in refused.stderr
    unknown = str(tmp_path / "unknown")
    _write_tree(unknown, raw_frames[:1], cal, models=("kb3", "kb3"))
    refused = subprocess.run([built, unknown, str(NF), "--rectify"], capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1 and "kb3" in refused.stderr
