"""Mesh of the volume on the MI355X (aria_mesh_*, kernels in aria_slam_amd/csrc/tsdf_mesh.hip) against its definition, the
NumPy restatement aria_slam_amd/mesh_ref.py: every vertex and triangle byte and both count words are BYTEWISE equal. The
build rounds every fp32 operation once and contracts nothing, so a difference is a bug, never a tolerance. The record volumes
are those of tests/mesh_cases.py, uploaded straight from torch tensors unless a test says otherwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_cases as MC   # noqa: E402
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import mesh as mesh_mod   # noqa: E402
from aria_slam_amd import mesh_ref as M   # noqa: E402

ARIA_E_INVALID, ARIA_E_OUTPUT_TOO_SMALL = -1, -5
PAD = 9                                                              # guard records behind each output


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def work(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return s


def _dev(torch, work, a):
    with torch.cuda.stream(work):
        t = torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to("cuda:0")       # a copy: the shared cases are read-only
    work.synchronize()
    return t


def _handle(aria, cfg, stream):
    return aria.HipVolumeMesher(dims=cfg.dims, voxel=cfg.voxel, origin=cfg.origin, min_weight=cfg.min_weight, stream=stream)


def _extract(torch, work, h, vcap, tcap, null_when_zero=False):
    """One extract into guarded device buffers of vcap + PAD and tcap + PAD records: (vertices, triangles, counts, status),
    the arrays with their guard records."""
    d_v = _dev(torch, work, np.full(16 * (vcap + PAD), MC.GUARD, np.uint8))
    d_t = _dev(torch, work, np.full(12 * (tcap + PAD), MC.GUARD, np.uint8))
    d_n = _dev(torch, work, np.full(16, MC.GUARD, np.uint8))
    h.extract_device(None if null_when_zero and vcap == 0 else d_v, vcap, None if null_when_zero and tcap == 0 else d_t, tcap, d_n)
    status = h.status()
    return (d_v.cpu().numpy().view(M.VERTEX_DTYPE), d_t.cpu().numpy().view(M.TRIANGLE_DTYPE),
            tuple(int(v) for v in d_n.cpu().numpy().view(np.int64)), status)


def _check(got, want, vcap, tcap):
    """The first min(total, cap) records equal the restatement's, everything behind them is guard bytes, counts are the totals."""
    gv, gt, counts, status = got
    wv, wt, (nv, nt) = want
    assert counts == (nv, nt)
    kv, kt = min(nv, vcap), min(nt, tcap)
    assert gv[:kv].tobytes() == wv[:kv].tobytes(), "vertices differ: %d of %d" % (int((gv[:kv] != wv[:kv]).sum()), kv)
    assert gt[:kt].tobytes() == wt[:kt].tobytes(), "triangles differ: %d of %d" % (int((gt[:kt] != wt[:kt]).sum()), kt)
    assert set(gv[kv:].tobytes()) <= {MC.GUARD} and set(gt[kt:].tobytes()) <= {MC.GUARD}, "a record beyond the written ones was touched"
    assert status == (ARIA_E_OUTPUT_TOO_SMALL if nv > vcap or nt > tcap else 0)


def _run(torch, work, aria, cfg, vol, want):
    h = _handle(aria, cfg, work.cuda_stream)
    try:
        h.update(_keep := _dev(torch, work, vol))
        nv, nt = want[2]
        got = _extract(torch, work, h, nv, nt)
        _check(got, want, nv, nt)
        return got
    finally:
        h.close()


def test_fused_scene_from_volume_and_the_axis_subset(torch_cuda, work, aria):
    """(a) HipTsdfVolume on the three-pose scene at 32 x 24 x 16, HipVolumeMesher.from_volume, no host copy of the volume: both
    arrays equal mesh_ref on the fusion restatement's records, and the vertices with dir 1, 2, 4 are, in order, the points
    extract_points_device gives for the same volume."""
    tcfg, _, pts = TC.ref_scene()
    d, im, e = TC.scene_frames()
    vol = aria.HipTsdfVolume(dims=tcfg.dims, voxel=tcfg.voxel, origin=tcfg.origin, trunc=tcfg.trunc, min_depth=tcfg.min_depth,
                             max_depth=tcfg.max_depth, max_weight=tcfg.max_weight, min_weight=tcfg.min_weight, K=tcfg.K,
                             stream=work.cuda_stream)
    h = None
    try:
        keep = [_dev(torch_cuda, work, np.ascontiguousarray(a)) for a in (d, e, im)]
        vol.integrate_batch_device(keep[0], TC.W, TC.H, keep[1], len(e), None, keep[2])
        assert vol.status() == 0
        h = aria.HipVolumeMesher.from_volume(vol, stream=work.cuda_stream)
        cfg, rec = MC.scene()
        assert h.ref_config == cfg
        want = MC.ref("scene", rec, cfg)
        nv, nt = want[2]
        got = _extract(torch_cuda, work, h, nv, nt)
        _check(got, want, nv, nt)
        assert nv > 1000 and nt > 1000
        d_p = _dev(torch_cuda, work, np.zeros(16 * len(pts), np.uint8))
        d_c = _dev(torch_cuda, work, np.zeros(8, np.uint8))
        vol.extract_points_device(d_p, len(pts), d_c)
        assert vol.status() == 0 and int(d_c.cpu().numpy().view(np.int64)[0]) == len(pts)
        points = d_p.cpu().numpy().view(TC.R.POINT_DTYPE)
        axis = got[0][:nv][np.isin(got[0][:nv]["dir"], (1, 2, 4))]
        assert len(axis) == len(points) > 400
        assert axis["X"].tobytes() == points["X"].tobytes() and (axis["gray"] == points["gray"]).all()
        assert (axis["weight"] == points["weight"]).all() and (axis["dir"] == 1 << points["axis"]).all()
        # the blocking host form and the counts
        hv, ht = h.extract()
        assert hv.tobytes() == want[0].tobytes() and ht.tobytes() == want[1].tobytes() and h.count() == (nv, nt)
    finally:
        if h is not None:
            h.close()
        vol.close()


@pytest.mark.parametrize("unseen", [0.0, 0.15])
def test_smallest_volume_special_values(torch_cuda, work, aria, unseen):
    """(b) 8 x 8 x 8: random tsdf with exact zeros, -0.0f and values one ulp either side of zero; weights min_weight - 1,
    min_weight and 65535; guarded outputs."""
    dims = (8, 8, 8)
    cfg, vol, want = MC.random_case(dims, unseen)
    assert set(np.unique(vol["weight"])) == ({MC.MIN_WEIGHT - 1} if unseen else set()) | {MC.MIN_WEIGHT, 65535}
    assert (vol["tsdf"] == 0).sum() > 10 and np.signbit(vol["tsdf"][vol["tsdf"] == 0]).any()
    _run(torch_cuda, work, aria, cfg, vol, want)
    assert want[2][0] > 200 and want[2][1] > 100


@pytest.mark.parametrize("dims", [(16, 16, 16), (24, 8, 16)])
def test_neighbours_in_other_chunks(torch_cuda, work, aria, dims):
    """(c) more than one chunk of 256 voxels in every direction a neighbour can lie, and dims that differ so that an index
    transposition shows."""
    cfg, vol, want = MC.random_case(dims, 0.15)
    _run(torch_cuda, work, aria, cfg, vol, want)


@pytest.mark.parametrize("dims,chunks", [((72, 64, 64), 1024), ((104, 104, 104), 4096)])
def test_second_scan_batch_and_its_carry(torch_cuda, work, aria, dims, chunks):
    """(d) 72 x 64 x 64 = 1152 chunks, more than the scan's 1024 lanes, and 104 x 104 x 104 = 4394 chunks, more than the 4096 of
    its first batch (a lane takes 4 chunks): the second batch and the carry into it. A thin shell, so mesh_ref stays fast."""
    cfg, vol = MC.config(dims), MC.shell_records(dims)
    want = MC.ref("shell_%r" % (dims,), vol, cfg)
    got = _run(torch_cuda, work, aria, cfg, vol, want)
    nv, nt = want[2]
    assert nv > 5000 and nt > 5000 and int(got[1][:nt]["v"].max()) < nv
    # voxels beyond `chunks` chunks own vertices
    lin_last = np.flatnonzero((vol["weight"] >= cfg.min_weight).reshape(-1)).max()
    assert lin_last // 256 >= chunks


def test_capacities_below_the_totals(torch_cuda, work, aria):
    """(e) vcap and tcap below the totals, alone and together, 0 and NULL: the counts hold the totals, the guard bytes are
    untouched, triangles keep the full numbering, and ARIA_E_OUTPUT_TOO_SMALL is reported once."""
    dims = (16, 16, 16)
    cfg, vol, want = MC.random_case(dims, 0.15)
    nv, nt = want[2]
    h = _handle(aria, cfg, work.cuda_stream)
    try:
        h.update(_keep := _dev(torch_cuda, work, vol))
        for vcap, tcap, null in ((nv // 3, nt, False), (nv, nt // 3, False), (nv // 2 + 1, nt // 2 + 1, False), (1, 1, False),
                                 (0, nt, False), (nv, 0, False), (0, 0, False), (0, nt, True), (nv, 0, True), (0, 0, True),
                                 (nv + 3, nt + 3, False)):
            got = _extract(torch_cuda, work, h, vcap, tcap, null)
            _check(got, want, vcap, tcap)
            assert h.status() == 0                                   # reported once
        cut_v, cut_t, totals = h.extract(vcap=5, tcap=7)
        assert totals == (nv, nt) and cut_v.tobytes() == want[0][:5].tobytes() and cut_t.tobytes() == want[1][:7].tobytes()
    finally:
        h.close()


def test_empty_volume_and_min_weight_above_every_weight(torch_cuda, work, aria):
    """(f) nothing to mesh: counts 0, nothing written, ARIA_OK."""
    dims = (16, 16, 16)
    empty = np.zeros(dims[::-1], M.VOXEL_DTYPE)
    full = MC.random_records(dims, seed=31, unseen=0.0, special=False).copy()
    full["weight"] = 40
    for vol, mw in ((empty, MC.MIN_WEIGHT), (full, 41)):
        cfg = MC.config(dims, min_weight=mw)
        h = _handle(aria, cfg, work.cuda_stream)
        try:
            h.update(_keep := _dev(torch_cuda, work, vol))
            got = _extract(torch_cuda, work, h, 4, 4)
            assert got[2] == (0, 0) and got[3] == 0 and set(got[0].tobytes()) | set(got[1].tobytes()) == {MC.GUARD}
            assert h.count() == (0, 0)
            v, t = h.extract()
            assert len(v) == 0 and len(t) == 0
        finally:
            h.close()
    assert M.extract(full, MC.config(dims, min_weight=40))[2][0] > 0


def test_identical_bytes_across_runs_handles_and_streams(torch_cuda, work, aria):
    """(g) twice on one handle, on a second handle with its own stream, and on a borrowed stream."""
    dims = (24, 8, 16)
    cfg, vol, want = MC.random_case(dims, 0.15)
    nv, nt = want[2]
    d_vol = _dev(torch_cuda, work, vol)
    a, b = _handle(aria, cfg, work.cuda_stream), _handle(aria, cfg, None)
    try:
        assert a.stream == work.cuda_stream and b.stream not in (None, work.cuda_stream)
        a.update(d_vol)
        first, second = _extract(torch_cuda, work, a, nv, nt), _extract(torch_cuda, work, a, nv, nt)
        b.update(d_vol)
        other = _extract(torch_cuda, work, b, nv, nt)
        a.update(d_vol)
        third = _extract(torch_cuda, work, a, nv, nt)
        for got in (first, second, other, third):
            _check(got, want, nv, nt)
    finally:
        a.close()
        b.close()


def test_refusals(torch_cuda, work, aria):
    """(h) extract before update; NULL handle and pointers; a capacity without its pointer; update holds the records and
    refuses a volume of another geometry."""
    L = aria.load_library()
    dims = (8, 8, 8)
    cfg, vol = MC.config(dims), MC.random_records(dims, seed=8)
    h = _handle(aria, cfg, work.cuda_stream)
    tcfg = TC.small_config()
    kw = dict(dims=tcfg.dims, trunc=tcfg.trunc, min_depth=tcfg.min_depth, max_depth=tcfg.max_depth, max_weight=tcfg.max_weight,
              min_weight=tcfg.min_weight, K=tcfg.K, stream=work.cuda_stream)
    same = aria.HipTsdfVolume(voxel=cfg.voxel, origin=cfg.origin, **kw)
    moved = aria.HipTsdfVolume(voxel=cfg.voxel, origin=(0.0, 0.0, 0.0), **kw)
    try:
        d_n = _dev(torch_cuda, work, np.full(16, MC.GUARD, np.uint8))
        d_v = _dev(torch_cuda, work, np.full(16 * 4, MC.GUARD, np.uint8))
        n = (C.c_int64 * 2)()
        assert L.aria_mesh_extract_device(h._h, None, 0, None, 0, d_n.data_ptr()) == ARIA_E_INVALID      # before the first update
        assert L.aria_mesh_extract(h._h, None, 0, None, 0, n) == ARIA_E_INVALID
        assert L.aria_mesh_update_from_volume_device(h._h, None) == ARIA_E_INVALID
        assert L.aria_mesh_update_from_volume_device(None, d_v.data_ptr()) == ARIA_E_INVALID
        h.update(_dev(torch_cuda, work, vol))                        # no other reference to the tensor
        assert h._records is not None
        for args in ((None, 0, None, 0, None), (None, 4, None, 0, d_n.data_ptr()), (None, 0, None, 4, d_n.data_ptr()),
                     (d_v.data_ptr(), -1, None, 0, d_n.data_ptr()), (None, 0, d_v.data_ptr(), -1, d_n.data_ptr())):
            assert L.aria_mesh_extract_device(h._h, *args) == ARIA_E_INVALID, args
        assert L.aria_mesh_extract_device(None, None, 0, None, 0, d_n.data_ptr()) == ARIA_E_INVALID
        assert h.status() == 0 and set(d_n.cpu().numpy().tobytes()) == {MC.GUARD}       # nothing was enqueued
        assert C.sizeof(type(h.config)) == 48
        with pytest.raises(ValueError):
            h.update(moved)
        h.update(same)
        assert h._records is same and h.count() == (0, 0)
    finally:
        h.close()
        assert h._records is None
        same.close()
        moved.close()


def test_export_ply_parses_back_to_the_arrays(torch_cuda, work, aria, tmp_path):
    """(i) the ASCII PLY: header, %.6g coordinates, r = g = b = gray, faces with the full numbering."""
    cfg, vol = MC.scene()
    want_v, want_t, (nv, nt) = MC.ref("scene", vol, cfg)
    h = _handle(aria, cfg, work.cuda_stream)
    try:
        h.update(_keep := _dev(torch_cuda, work, vol))
        path = str(tmp_path / "mesh.ply")
        h.export_ply(path)
    finally:
        h.close()
    text = open(path).read()
    assert text == mesh_mod.ply_text(want_v, want_t)
    assert text.startswith("ply\nformat ascii 1.0\nelement vertex %d\n" % nv)
    assert "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % nt in text
    X, gray, faces = mesh_mod.read_ply(path)
    # %.6g keeps six significant digits: half a unit of the sixth is at most 5e-6 of the value
    assert X.shape == (nv, 3) and np.allclose(X, want_v["X"], rtol=5e-6, atol=0) and (gray == want_v["gray"]).all()
    assert (faces == want_t["v"]).all()
