"""The C++ side of dense depth fusion on the MI355X: aria_hip/HipTsdfVolume.hpp wraps the stage and euroc_frontend --volume
integrates the --dense depth maps along the --pose chain and writes the surface points as PLY. Without --volume every other
output of the driver is byte-identical."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_stereo import BASELINE, FRAMES, NF, _frames, _run, _write_tree   # noqa: E402

PLY_HEAD = ["ply", "format ascii 1.0", None, "property float x", "property float y", "property float z", "property uchar red",
            "property uchar green", "property uchar blue", "end_header"]
NAMES = ("stereo.txt", "pose.txt", "frames.csv", "dense.txt")


def _common(f):
    return ["--stereo", BASELINE, "--stereo-out", f["stereo.txt"], "--pose", f["pose.txt"], "--csv", f["frames.csv"],
            "--dense", f["dense.txt"]]


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


def _volume_run(built, tmp_path, frames):
    """euroc_frontend --volume on a sequence; the checks that hold for any sequence. Returns (points, observed voxels, frames
    with a valid scale, the output files, the sequence root, the PLY path)."""
    from aria_slam_amd import mapper
    root = str(tmp_path / "seq")
    _write_tree(root, frames)
    with_flag = {k: str(tmp_path / ("v_" + k)) for k in NAMES}
    ply = str(tmp_path / "volume.ply")
    stdout = _run(built, root, NF, *_common(with_flag), "--volume", ply, "--voxel", 0.1)
    # exactly one line of the stage, "volume <points> <observed voxels>"
    line = [l for l in stdout.splitlines() if l.startswith("volume")]
    assert len(line) == 1 and line[0].startswith("volume ") and len(line[0].split()) == 3, line
    points, observed = (int(v) for v in line[0].split()[1:])
    # a well-formed PLY: HipMapper's header text, one vertex line per point in ostream's default format (what mapper.ply_text
    # writes as %.6g), r = g = b, inside the volume
    text = open(ply).read().splitlines(keepends=True)
    assert "".join(text[:len(PLY_HEAD)]) == mapper.PLY_HEADER.format(n=points) and len(text) == len(PLY_HEAD) + points
    half = (12.8, 12.8, 6.4)                                         # 256 x 256 x 128 voxels of 0.1 m centred on the first camera
    for l in text[len(PLY_HEAD):]:
        f = l.split()
        assert len(f) == 6 and f[3] == f[4] == f[5] and 0 <= int(f[3]) <= 255
        assert l == "%.6g %.6g %.6g %d %d %d\n" % (float(f[0]), float(f[1]), float(f[2]), int(f[3]), int(f[4]), int(f[5])), l
        assert all(abs(float(v)) <= h for v, h in zip(f[:3], half))
    scaled = sum(int(l.split()[3]) for l in open(with_flag["stereo.txt"]).read().splitlines())
    print("volume: %d points, %d observed voxels, %d of %d frames scaled" % (points, observed, scaled, FRAMES))
    assert observed >= points // 3
    return points, observed, scaled, with_flag, root, ply


def test_euroc_frontend_volume_writes_a_ply_and_changes_nothing_else(aria, built, tmp_path):
    """The sequence the other test_cpp_* files build (a window sliding over one pair)."""
    points, observed, scaled, with_flag, root, ply = _volume_run(built, tmp_path, _frames())
    # frames with an accepted pose and a valid scale exist on this sequence, so the driver's integrate path ran; the scene's
    # nearest row of rectangles (disparity 42.25, depth 458.654 * 0.25 / 42.25 = 2.7 m) lies inside the volume and in range, so
    # there is a surface
    assert scaled > 0 and points > 0 and observed > 0
    # every other output is byte-identical without the flag, and nothing of the stage is printed
    without = {k: str(tmp_path / ("p_" + k)) for k in NAMES}
    stdout = _run(built, root, NF, *_common(without))
    assert not any(l.startswith("volume") for l in stdout.splitlines())
    for k in NAMES:
        assert open(with_flag[k], "rb").read() == open(without[k], "rb").read(), k
    # --volume needs --pose, --stereo and --dense
    for args in (["--stereo", str(BASELINE), "--dense", with_flag["dense.txt"]], ["--pose", with_flag["pose.txt"]],
                 ["--stereo", str(BASELINE), "--pose", with_flag["pose.txt"]]):
        refused = subprocess.run([built, root, str(NF), "--volume", ply] + args, capture_output=True, text=True, timeout=300)
        assert refused.returncode != 0 and "--volume needs" in refused.stderr


def test_adapters_library_holds_the_volume_class(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipTsdfVolume::integrate", "aria::adapters::hip::HipTsdfVolume::extractPoints",
                 "aria::adapters::hip::HipTsdfVolume::exportPLY", "aria::adapters::hip::HipTsdfVolume::observedVoxels",
                 "aria::adapters::hip::TsdfVolumeConfig::centreOn"):
        assert name in syms, name
