"""The C++ side of ray casting on the MI355X: aria_hip/HipVolumeRenderer.hpp wraps the stage and euroc_frontend --volume FILE.ply
--render PREFIX casts the finished volume at every N-th integrated pose and writes a depth and a shade PGM per view. Without
--render every other output of the driver is byte-identical."""
import glob
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_stereo import BASELINE, H, NF, W, _frames, _run, _write_tree   # noqa: E402

NAMES = ("stereo.txt", "pose.txt", "frames.csv", "dense.txt", "volume.ply")


def _common(f):
    return ["--stereo", BASELINE, "--stereo-out", f["stereo.txt"], "--pose", f["pose.txt"], "--csv", f["frames.csv"],
            "--dense", f["dense.txt"], "--volume", f["volume.ply"], "--voxel", 0.1]


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


def test_euroc_frontend_render_writes_pgms_and_changes_nothing_else(aria, built, tmp_path):
    """The sequence the other test_cpp_* files build (a window sliding over one pair), on which --volume finds a surface."""
    from aria_slam_amd import render
    root = str(tmp_path / "seq")
    _write_tree(root, _frames())
    every = {k: str(tmp_path / ("e_" + k)) for k in NAMES}
    prefix = str(tmp_path / "every")
    stdout = _run(built, root, NF, *_common(every), "--render", prefix, "--render-every", 1)
    line = [l for l in stdout.splitlines() if l.startswith("render")]
    assert len(line) == 1 and line[0].startswith("render ") and len(line[0].split()) == 3, line
    n_views, hits = (int(v) for v in line[0].split()[1:])
    # the integrated frames are those with a valid scale (field 3 of the --stereo-out lines): one view each, named by the frame
    scaled = [i for i, l in enumerate(open(every["stereo.txt"]).read().splitlines()) if int(l.split()[3])]
    assert n_views == len(scaled) > 0 and hits > 0
    want = sorted("%s_%d_%s.pgm" % (prefix, i, kind) for i in scaled for kind in ("depth", "shade"))
    assert sorted(glob.glob(prefix + "_*")) == want
    counted = 0
    for i in scaled:
        depth, shade = render.read_pgm("%s_%d_depth.pgm" % (prefix, i)), render.read_pgm("%s_%d_shade.pgm" % (prefix, i))
        assert depth.shape == shade.shape == (H, W) and depth.dtype.itemsize == 2 and shade.dtype.itemsize == 1
        assert os.path.getsize("%s_%d_depth.pgm" % (prefix, i)) == len("P5\n%d %d\n65535\n" % (W, H)) + 2 * W * H
        assert os.path.getsize("%s_%d_shade.pgm" % (prefix, i)) == len("P5\n%d %d\n255\n" % (W, H)) + W * H
        hit = depth > 0
        counted += int(hit.sum())
        assert not shade[~hit].any() and depth[hit].min() >= 300 and depth.max() <= 10050       # millimetres between near and far
    assert counted == hits
    print("render: %d views, %d hit pixels of %d" % (n_views, hits, n_views * W * H))
    # the default: every tenth integrated pose, here the first alone
    tenth = {k: str(tmp_path / ("t_" + k)) for k in NAMES}
    prefix10 = str(tmp_path / "tenth")
    stdout = _run(built, root, NF, *_common(tenth), "--render", prefix10)
    line = [l for l in stdout.splitlines() if l.startswith("render")]
    assert len(line) == 1 and int(line[0].split()[1]) == 1
    assert sorted(glob.glob(prefix10 + "_*")) == sorted("%s_%d_%s.pgm" % (prefix10, scaled[0], kind) for kind in ("depth", "shade"))
    assert open("%s_%d_depth.pgm" % (prefix10, scaled[0]), "rb").read() == open("%s_%d_depth.pgm" % (prefix, scaled[0]), "rb").read()
    # every other output is byte-identical without the flag, and nothing of the stage is printed
    without = {k: str(tmp_path / ("p_" + k)) for k in NAMES}
    stdout = _run(built, root, NF, *_common(without))
    assert not any(l.startswith("render") for l in stdout.splitlines())
    for k in NAMES:
        assert open(every[k], "rb").read() == open(without[k], "rb").read() == open(tenth[k], "rb").read(), k
    # --render needs --volume
    refused = subprocess.run([built, root, str(NF), "--render", prefix], capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--render needs" in refused.stderr


def test_adapters_library_holds_the_renderer_class(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipVolumeRenderer::update", "aria::adapters::hip::HipVolumeRenderer::castBatch",
                 "aria::adapters::hip::HipVolumeRenderer::castBatchDevice", "aria::adapters::hip::HipVolumeRenderer::writeDepthPGM",
                 "aria::adapters::hip::VolumeRendererConfig::fromVolume"):
        assert name in syms, name
