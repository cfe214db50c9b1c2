"""The kernel source of aria_slam_amd/csrc/tsdf_mesh.hip, compiled for the HOST and held bytewise to the restatement
(aria_slam_amd/mesh_ref.py).

The text of the file between "namespace {" and the kernels section -- mesh_voxel, mesh_vertex, mesh_vertex_number,
mesh_cell_triangles, mesh_count_errors and the table -- is pasted between tests/cpp/mesh_kernel_emu_head.inc (a shim) and
mesh_kernel_emu_tail.inc (the three passes with the lanes of every chunk taken in order) and compiled with the clang++ that
hipcc drives. What this checks without a GPU is the indexing, the parked word, the numbering of a neighbour's vertex from
that word and the chunk offsets, the table lookups and the order of the fp32 operations as the host compiler takes them; what
it cannot check is the device's arithmetic, the scans across lanes and the streams: that is tests/test_gpu_mesh.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_cases as MC   # noqa: E402


@pytest.mark.parametrize("dims", [(8, 8, 8), (24, 8, 16)])
@pytest.mark.parametrize("unseen", [0.0, 0.15])
def test_mesh_kernel_source_is_bytewise_the_restatement_on_random_records(dims, unseen):
    """Random records with exact zeros, -0.0f and values one ulp either side of zero; with a share of unseen voxels the
    cells around them are not live while their edges still carry vertices."""
    cfg, vol, (want_v, want_t, (nv, nt)) = MC.random_case(dims, unseen)
    got_v, got_t, totals, bits = MC.emu_extract(vol, cfg)
    assert bits == 0 and totals == (nv, nt) and nv > 200 and nt > 100
    assert got_v.tobytes() == want_v.tobytes(), int((got_v != want_v).sum())
    assert got_t.tobytes() == want_t.tobytes(), int((got_t != want_t).sum())
    assert set(want_v["dir"]) == set(range(1, 8))


def test_mesh_kernel_source_on_the_fused_scene_and_the_capacity_cut():
    """The three-pose scene as the fusion leaves it (weights 0..3, a truncation band), then capacities below the totals: the
    first records, the full numbering, the totals, bit 1, and nothing written past the capacity."""
    cfg, vol = MC.scene()
    want_v, want_t, (nv, nt) = MC.ref("scene", vol, cfg)
    got_v, got_t, totals, bits = MC.emu_extract(vol, cfg)
    assert bits == 0 and totals == (nv, nt) and nv > 1000 and nt > 1000
    assert got_v.tobytes() == want_v.tobytes() and got_t.tobytes() == want_t.tobytes()
    for vcap, tcap in ((nv // 3, nt + 5), (nv + 5, nt // 3), (7, 5), (0, nt), (nv, 0)):
        got_v, got_t, totals, bits = MC.emu_extract(vol, cfg, vcap, tcap)
        assert totals == (nv, nt) and bits == (1 if vcap < nv or tcap < nt else 0)
        assert got_v[:min(vcap, nv)].tobytes() == want_v[:vcap].tobytes() and got_t[:min(tcap, nt)].tobytes() == want_t[:tcap].tobytes()
        assert set(got_v[nv:].tobytes()) <= {MC.GUARD} and set(got_t[nt:].tobytes()) <= {MC.GUARD}


def test_mesh_kernel_source_empty_and_unseen_volumes():
    cfg = MC.config((8, 8, 8))
    vol = np.zeros((8, 8, 8), MC.M.VOXEL_DTYPE)
    assert MC.emu_extract(vol, cfg)[2:] == ((0, 0), 0)
    vol = MC.random_records((8, 8, 8), seed=5).copy()
    vol["weight"] = MC.MIN_WEIGHT - 1
    assert MC.emu_extract(vol, cfg)[2:] == ((0, 0), 0)
