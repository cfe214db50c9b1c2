"""The C++ side of path planning on the MI355X: aria_hip/HipPathPlanner.hpp wraps the stage and euroc_frontend --plan plans over
the --volume map from the cell under the first camera of the --pose chain to the cell under the last. Without --plan every
other output of the driver is byte-identical."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_stereo import BASELINE, NF, _frames, _run, _write_tree   # noqa: E402
from aria_slam_amd import nav_ref as R   # noqa: E402

NAMES = ("stereo.txt", "pose.txt", "frames.csv", "dense.txt", "volume.ply")
VOXEL = 0.1


def _common(f):
    return ["--stereo", BASELINE, "--stereo-out", f["stereo.txt"], "--pose", f["pose.txt"], "--csv", f["frames.csv"],
            "--dense", f["dense.txt"], "--volume", f["volume.ply"], "--voxel", VOXEL]


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


def _centres(pose_file):
    """The camera centres -R^T t of the first and the last line of a TUM file of world-to-camera poses."""
    out = []
    lines = open(pose_file).read().splitlines()
    for l in (lines[0], lines[-1]):
        _, tx, ty, tz, qx, qy, qz, qw = (float(v) for v in l.split())
        Rm = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                       [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                       [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
        out.append(-Rm.T @ np.array([tx, ty, tz]))
    return out


def test_euroc_frontend_plan_writes_a_path_and_changes_nothing_else(aria, built, tmp_path):
    root = str(tmp_path / "seq")
    _write_tree(root, _frames())
    with_flag = {k: str(tmp_path / ("n_" + k)) for k in NAMES}
    path_file = str(tmp_path / "path.txt")
    stdout = _run(built, root, NF, *_common(with_flag), "--plan", path_file)
    # exactly one line of the stage, "plan <status> <cost> <cells>"
    line = [l for l in stdout.splitlines() if l.startswith("plan")]
    assert len(line) == 1 and line[0].startswith("plan ") and len(line[0].split()) == 4, line
    status, cost, cells = (int(v) for v in line[0].split()[1:])
    print(line[0])
    pts = [[float(v) for v in l.split()] for l in open(path_file).read().splitlines()]
    assert len(pts) == cells and all(len(p) == 3 for p in pts)
    # the volume of the driver: 256 x 256 x 128 voxels of --voxel metres centred on the first camera, the world origin
    cfg = R.config(voxel=VOXEL, origin=(-12.8, -12.8, -6.4))
    first, last = (R.cell_of(c[None], cfg)[0] for c in _centres(with_flag["pose.txt"]))
    nu, nv = R.grid_shape(cfg)
    assert all(0 <= c[0] < nu and 0 <= c[1] < nv for c in (first, last))
    # this tree is deterministic: the stereo scale moves the camera over several cells of 0.1 m, both camera cells lie inside
    # the grid and the ground between them is free or unseen (UNKNOWN is allowed by default), so there IS a path of several cells
    assert status == R.OK and tuple(first) != tuple(last)
    assert cells >= 2 and cells >= 1 + max(abs(int(last[0] - first[0])), abs(int(last[1] - first[1])))
    assert 10 * (cells - 1) <= cost < R.INF                          # every step costs at least 10
    # the first and last lines are centre_of of the first and last camera cells, printed with nine digits: exact in fp32
    assert np.array(pts[0], np.float32).tolist() == R.centre_of(first, cfg)[0].tolist()
    assert np.array(pts[-1], np.float32).tolist() == R.centre_of(last, cfg)[0].tolist()
    # consecutive lines differ by at most one voxel on each plane axis, by something, and not at all on the up axis
    got = R.cell_of(np.array(pts, np.float32), cfg)
    step = np.abs(np.diff(got, axis=0))
    assert step.max() <= 1 and (step.sum(axis=1) >= 1).all() and len(set(p[1] for p in pts)) == 1
    assert np.array(pts, np.float32).tolist() == R.centre_of(got, cfg).tolist()
    # every other output is byte-identical without the flag, and nothing of the stage is printed
    without = {k: str(tmp_path / ("p_" + k)) for k in NAMES}
    stdout2 = _run(built, root, NF, *_common(without))
    assert not any(l.startswith("plan") for l in stdout2.splitlines())
    for k in NAMES:
        assert open(with_flag[k], "rb").read() == open(without[k], "rb").read(), k
    # --plan needs --volume
    refused = subprocess.run([built, root, str(NF), "--plan", path_file, "--pose", with_flag["pose.txt"]], capture_output=True, text=True,
                             timeout=300)
    assert refused.returncode != 0 and "--plan needs" in refused.stderr


def test_adapters_library_holds_the_planner_class(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipPathPlanner::plan", "aria::adapters::hip::HipPathPlanner::update",
                 "aria::adapters::hip::HipPathPlanner::cellOf", "aria::adapters::hip::HipPathPlanner::centreOf",
                 "aria::adapters::hip::PathPlannerConfig::fromVolume"):
        assert name in syms, name
