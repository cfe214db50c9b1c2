"""The C++ side of dense stereo on the MI355X: aria_hip/HipDenseStereo.hpp wraps the stage and euroc_frontend --dense writes
per frame the valid share and the median depth of the map the restatement (aria_slam_amd/dense_ref.py) defines for the same
images. Without --dense every other output of the driver is byte-identical."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_stereo import BASELINE, FRAMES, NF, T0, _frames, _run, _write_tree   # noqa: E402


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


def _restatement_lines(frames):
    from aria_slam_amd import dense_ref as R
    lines = []
    for f, (left, right) in enumerate(frames):
        d16 = R.dense_disparity(left, right)
        z = np.sort(R.depth_map(d16, R.EUROC_K, BASELINE)[d16 > 0])
        lines.append("%.9f %.9f %.9f" % ((T0 + f * 50_000_000) * 1e-9, float((d16 > 0).sum()) / d16.size,
                                         float(z[len(z) // 2]) if len(z) else 0.0))
    return lines


def test_euroc_frontend_dense_lines_equal_the_restatement(aria, built, tmp_path):
    frames = _frames()
    root = str(tmp_path / "seq")
    _write_tree(root, frames)
    with_flag = {k: str(tmp_path / ("d_" + k)) for k in ("stereo.txt", "pose.txt", "frames.csv")}
    without = {k: str(tmp_path / ("p_" + k)) for k in with_flag}
    dense_out = str(tmp_path / "dense.txt")
    common = lambda f: ["--stereo", BASELINE, "--stereo-out", f["stereo.txt"], "--pose", f["pose.txt"], "--csv", f["frames.csv"]]   # noqa: E731
    stdout = _run(built, root, NF, *common(with_flag), "--dense", dense_out)
    assert "dense 64 disparities" in stdout
    got = open(dense_out).read().splitlines()
    want = _restatement_lines(frames)
    assert got == want
    assert len(got) == FRAMES and all(float(l.split()[1]) > 0.5 and float(l.split()[2]) > 0 for l in got)
    # every other output is byte-identical without the flag, and nothing of the stage is printed
    stdout = _run(built, root, NF, *common(without))
    assert not any(l.startswith("dense ") for l in stdout.splitlines())
    for k in with_flag:
        assert open(with_flag[k], "rb").read() == open(without[k], "rb").read(), k
    # --dense needs --stereo for cam1 and the baseline
    refused = subprocess.run([built, root, str(NF), "--dense", dense_out], capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--stereo" in refused.stderr


def test_adapters_library_holds_the_dense_class(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipDenseStereo::compute", "aria::adapters::hip::HipDenseStereo::sample",
                 "aria::adapters::hip::DenseDepth::medianDepth", "aria::adapters::hip::DenseDepth::validShare"):
        assert name in syms, name
