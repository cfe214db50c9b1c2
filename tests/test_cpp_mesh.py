"""The C++ side of the mesh stage on the MI355X: aria_hip/HipVolumeMesher.hpp wraps the stage and euroc_frontend --mesh
contours the --volume map and writes the triangle mesh as PLY after the volume's points. Without --mesh every other output of
the driver is byte-identical."""
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
from test_cpp_tsdf import NAMES, _common   # noqa: E402
from aria_slam_amd import mesh as mesh_mod   # noqa: E402
from aria_slam_amd import mesh_ref   # noqa: E402


@pytest.fixture(scope="module")
def built(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    return os.path.join(PKG, "euroc_frontend")


def test_euroc_frontend_mesh_writes_a_ply_and_changes_nothing_else(aria, built, tmp_path):
    """The sequence the other test_cpp_* files build. The mesh PLY parses, its counts are the printed ones, its axis vertices
    are the --volume file's points line for line, every face index is in range and no directed edge occurs twice."""
    root = str(tmp_path / "seq")
    _write_tree(root, _frames())
    with_flag = {k: str(tmp_path / ("m_" + k)) for k in NAMES}
    ply, mesh = str(tmp_path / "volume.ply"), str(tmp_path / "mesh.ply")
    stdout = _run(built, root, NF, *_common(with_flag), "--volume", ply, "--voxel", 0.1, "--mesh", mesh)
    line = [l for l in stdout.splitlines() if l.startswith("mesh")]
    assert len(line) == 1 and len(line[0].split()) == 3, line
    nv, nt = (int(v) for v in line[0].split()[1:])
    points = int([l for l in stdout.splitlines() if l.startswith("volume ")][0].split()[1])
    text = open(mesh).read().splitlines()
    end = text.index("end_header")
    assert text[:end + 1] == mesh_mod.ply_text(np.zeros(nv, mesh_ref.VERTEX_DTYPE), np.zeros(0, mesh_ref.TRIANGLE_DTYPE)).replace(
        "element face 0", "element face %d" % nt).splitlines()[:end + 1]
    assert len(text) == end + 1 + nv + nt
    X, gray, faces = mesh_mod.read_ply(mesh)
    print("mesh: %d vertices, %d triangles, %d volume points" % (nv, nt, points))
    assert nv > points > 0 and nt > 0 and X.shape == (nv, 3) and faces.shape == (nt, 3)
    assert faces.min() >= 0 and faces.max() < nv
    assert mesh_ref.edge_report(faces)[0] == 0
    for l in text[end + 1:end + 1 + nv]:
        f = l.split()
        assert len(f) == 6 and f[3] == f[4] == f[5]
        assert l == "%.6g %.6g %.6g %d %d %d" % (float(f[0]), float(f[1]), float(f[2]), int(f[3]), int(f[4]), int(f[5])), l
    # the volume's points are a subset of the mesh's vertex lines, in order (rule 2: dir 1, 2, 4)
    vertex_lines = iter(text[end + 1:end + 1 + nv])
    for l in open(ply).read().splitlines()[10:]:
        assert any(l == m for m in vertex_lines), "a surface point is missing from the mesh vertices, or out of order"
    # every other output is byte-identical without the flag, the volume's PLY included, and nothing of the stage is printed
    without = {k: str(tmp_path / ("p_" + k)) for k in NAMES}
    ply2 = str(tmp_path / "volume2.ply")
    stdout2 = _run(built, root, NF, *_common(without), "--volume", ply2, "--voxel", 0.1)
    assert not any(l.startswith("mesh") for l in stdout2.splitlines())
    for k in NAMES:
        assert open(with_flag[k], "rb").read() == open(without[k], "rb").read(), k
    assert open(ply, "rb").read() == open(ply2, "rb").read()
    # --mesh needs --volume
    refused = subprocess.run([built, root, str(NF), "--mesh", mesh, "--stereo", str(BASELINE), "--pose", with_flag["pose.txt"],
                              "--dense", with_flag["dense.txt"]], capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--mesh needs" in refused.stderr


def test_adapters_library_holds_the_mesher_class(built):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "libaria_hip_adapters.so")], capture_output=True, text=True,
                          check=True).stdout
    for name in ("aria::adapters::hip::HipVolumeMesher::update", "aria::adapters::hip::HipVolumeMesher::extract",
                 "aria::adapters::hip::HipVolumeMesher::exportPLY", "aria::adapters::hip::HipVolumeMesher::count",
                 "aria::adapters::hip::VolumeMesherConfig::fromVolume"):
        assert name in syms, name
