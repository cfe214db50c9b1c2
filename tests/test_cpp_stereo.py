"""The C++ side of sparse stereo on the MI355X: AslSequence pairs mav0/cam1 with cam0, aria_hip/HipStereoMatcher.hpp wraps
the stage, and euroc_frontend --stereo prints per frame what the Python binding computes from the same images. Without
--stereo the driver's outputs do not change, with or without a cam1 directory in the tree."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

W, H, NF, FRAMES, BASELINE = 320, 240, 500, 4, 0.25
T0 = 1403636579763555584


def _frames():
    """Four rectified pairs: a 328-px-wide stereo_scene pair seen through a window that moves 2 px per frame."""
    from aria_slam_amd import stereo_ref as R
    left, right, _ = R.stereo_pair(11, W + 2 * FRAMES, H)
    return [(np.ascontiguousarray(left[:, 2 * f:2 * f + W]), np.ascontiguousarray(right[:, 2 * f:2 * f + W])) for f in range(FRAMES)]


def _write_tree(root, frames, cam1=True):
    from test_frontend_io import write_png
    for cam, side in (("cam0", 0), ("cam1", 1)):
        if cam == "cam1" and not cam1:
            continue
        d = os.path.join(root, "mav0", cam, "data")
        os.makedirs(d, exist_ok=True)
        rows = []
        for f, pair in enumerate(frames):
            ts = T0 + f * 50_000_000
            open(os.path.join(d, "%d.png" % ts), "wb").write(write_png(pair[side]))
            rows.append("%d,%d.png" % (ts, ts))
        if cam == "cam1":
            rows = rows[::-1] + ["%d,%d.png" % (T0 + 25_000_000, T0)]         # unsorted, and one image without a cam0 partner
        with open(os.path.join(root, "mav0", cam, "data.csv"), "w") as fh:
            fh.write("#timestamp [ns],filename\n" + "\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _python_lines(aria, frames, with_pose):
    """What euroc_frontend --stereo computes, through the Python binding: query = current frame, train = previous."""
    ext = aria.OrbHipExtractor(max_features=NF, max_width=W, max_height=H)
    mat = aria.HipMatcher()
    pe = aria.HipPoseEstimator()
    st = aria.HipStereoMatcher(baseline=BASELINE)
    lines, prev, prev_obs = [], None, None
    try:
        for f, (left, right) in enumerate(frames):
            cur, rf = ext.extract(left), ext.extract(right)
            obs, m = st.match(left, right, cur, rf)
            depth = np.sort(obs["depth"][obs["right_idx"] >= 0])
            line = "%.9f %d %.9f" % ((T0 + f * 50_000_000) * 1e-9, len(m), float(depth[len(depth) // 2]) if len(depth) else 0.0)
            if with_pose:
                valid, scale = 0, 1.0
                if prev is not None:
                    mm = mat.match(cur, prev, None, 0.75)
                    if len(mm) >= 8:
                        pose = pe.estimate(cur, prev, mm, query_is_first=False, pair_base=f)
                        if pose["valid"] and pose["n_pose_inliers"] > 10:
                            s = st.scale(pose, mm, obs, prev_obs, query_is_first=False)
                            valid, scale = int(s["valid"]), float(s["scale"])
                line += " %d %.9f" % (valid, scale)
            lines.append(line)
            prev, prev_obs = cur, obs
    finally:
        for h in (st, pe, mat, ext):
            h.close()
    return lines


def test_euroc_frontend_stereo_lines_equal_the_python_binding(aria, built, tmp_path):
    frames = _frames()
    root = str(tmp_path / "seq")
    _write_tree(root, frames)
    # the reader pairs by equal timestamp, whatever the order of cam1's rows
    L = C.CDLL(os.path.join(PKG, "libaria_hip_adapters.so"))
    L.aria_asl_stereo.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    has = np.zeros(8, np.int32)
    assert L.aria_asl_stereo(root.encode(), has.ctypes.data, 8) == FRAMES and list(has[:FRAMES]) == [1] * FRAMES
    out_a, out_b, pose = (str(tmp_path / n) for n in ("stereo.txt", "stereo_pose.txt", "pose.txt"))
    stdout = _run(built, root, NF, "--stereo", BASELINE, "--stereo-out", out_a)
    assert "stereo baseline 0.25 m" in stdout
    got = open(out_a).read().splitlines()
    want = _python_lines(aria, frames, False)
    assert got == want
    assert all(int(l.split()[1]) > 100 and float(l.split()[2]) > 0 for l in got)
    # with --pose: the scale columns; to the standard output without --stereo-out
    _run(built, root, NF, "--stereo", BASELINE, "--stereo-out", out_b, "--pose", pose)
    got = open(out_b).read().splitlines()
    want = _python_lines(aria, frames, True)
    assert got == want
    stdout = _run(built, root, NF, "--stereo", BASELINE)
    assert [l[len("stereo "):] for l in stdout.splitlines() if l.startswith("stereo 14")] == _python_lines(aria, frames, False)
    # bad uses are refused
    for bad in (["--stereo", "0"], ["--stereo-out", out_a], ["--stereo", "0.1", "--batch", "2"]):
        assert subprocess.run([built, root, str(NF)] + bad, capture_output=True, text=True, timeout=300).returncode != 0


def test_outputs_without_stereo_do_not_change(aria, built, tmp_path):
    """The same frames with and without a cam1 directory: --pose and --csv are byte-identical, and a --stereo run leaves the
    per-frame hashes of the CSV as they are. A tree without cam1 refuses --stereo."""
    frames = _frames()
    with_cam1, without = str(tmp_path / "a"), str(tmp_path / "b")
    _write_tree(with_cam1, frames)
    _write_tree(without, frames, cam1=False)
    files = {}
    for tag, root in (("a", with_cam1), ("b", without)):
        files[tag] = (str(tmp_path / (tag + "_pose.txt")), str(tmp_path / (tag + ".csv")))
        _run(built, root, NF, "--pose", files[tag][0], "--csv", files[tag][1])
    assert open(files["a"][0], "rb").read() == open(files["b"][0], "rb").read()
    assert open(files["a"][1], "rb").read() == open(files["b"][1], "rb").read()
    assert len(open(files["a"][0]).read().splitlines()) == FRAMES
    csv2 = str(tmp_path / "s.csv")
    _run(built, with_cam1, NF, "--stereo", BASELINE, "--csv", csv2, "--stereo-out", str(tmp_path / "s.txt"))
    plain = str(tmp_path / "p.csv")
    _run(built, with_cam1, NF, "--csv", plain)
    assert open(csv2, "rb").read() == open(plain, "rb").read()
    refused = subprocess.run([built, without, str(NF), "--stereo", str(BASELINE)], capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "cam1" in refused.stderr
