"""Ray casting of the volume on the MI355X (aria_ray_*, kernels in aria_slam_amd/csrc/tsdf_raycast.hip) against its
definition, the NumPy restatement aria_slam_amd/ray_ref.py: every requested output byte and every view record is BITWISE
equal. The build rounds every fp32 operation once and contracts nothing, so a difference is a bug, never a tolerance. The
shapes are those of tests/ray_cases.py; the restatement neither clips nor skips, so every comparison on a grazing view tests
the clip bounds and every comparison at skip = 1 the brick bits.

Measured with the restatement (tests/test_ray_host.py asserts them): `half_behind` at the scene's own min_weight = 2 ends no
walk (n_ended 0: the far side of the sphere was seen by one frame only), so the assertion n_ended > 0 is made on the same
view at min_weight = 1 (172 walks end, none hits) and on `inside` (970 end, 76 hit); step 0.1 from 2.0 to 2.6 is 6 samples in
fp32 and gives 2459 hits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_cases as AC   # noqa: E402
import ray_cases as RC   # noqa: E402
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import alert_ref   # noqa: E402

ARIA_E_INVALID = -1
CASES = RC.all_cases()


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


def _handle(aria, work, cfg, skip=1):
    return aria.HipVolumeRenderer(dims=cfg.dims, voxel=cfg.voxel, origin=cfg.origin, min_weight=cfg.min_weight, near=cfg.near,
                                  far=cfg.far, step=cfg.step, skip=skip, K=cfg.K, stream=work.cuda_stream)


def _cast(torch, work, h, case, layout, planes=RC.PLANES, views=True):
    """One cast into guarded device buffers: ({plane: buffer, "views": records}, status)."""
    host = RC.guarded(case, layout, planes)
    dev = {k: _dev(torch, work, v) for k, v in host.items()}
    d_ext = _dev(torch, work, np.ascontiguousarray(case.ext, np.float64))
    d_mask = None if case.mask is None else _dev(torch, work, case.mask)
    kw = {}
    for p in RC.PLANES:
        kw["d_" + p] = dev[p] if p in planes else None
        kw[p + "_pitch"], kw[p + "_stride"] = layout[p]
    h.cast_batch_device(d_ext, len(case.ext), case.W, case.H, d_views=dev["views"] if views else None, d_view_mask=d_mask, **kw)
    status = h.status()
    return {k: dev[k].cpu().numpy().view(host[k].dtype).reshape(host[k].shape) for k in host}, status


def _run(torch, work, aria, case, layout, skip=1, **kw):
    h = _handle(aria, work, case.cfg, skip)
    try:
        d_vol = _dev(torch, work, case.vol)
        h.update(d_vol)
        return _cast(torch, work, h, case, layout, **kw)
    finally:
        h.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cast_equals_the_restatement_with_and_without_skipping(torch_cuda, work, aria, name):
    """Shapes (a), (b), (c) and the slab, and (d): skip = 1 and skip = 0 give the restatement's bytes, hence each other's."""
    case = CASES[name]
    layout = RC.dense_layout(case.W, case.H)
    want = RC.expected(case, layout)
    for skip in (1, 0):
        got, status = _run(torch_cuda, work, aria, case, layout, skip)
        diff = RC.same_bytes(got, want)
        print("%s skip %d: differing bytes %r, n_hit %r" % (name, skip, diff, [int(v) for v in want["views"]["n_hit"][:4]]))
        assert diff == {}
        assert status == (ARIA_E_INVALID if RC.ref(case)[1] else 0)
    if name == "frustum_half_behind_seen_once":
        assert int(want["views"][0]["n_ended"]) > 0 and int(want["views"][0]["n_hit"]) == 0
    if name == "frustum_inside":
        assert int(want["views"][0]["n_ended"]) > int(want["views"][0]["n_hit"]) > 0


def test_scene_batch_bad_view_masked_view_singles_and_rerun(torch_cuda, work, aria):
    """Shape (a): the bad view's planes are zero, its valid is 0 and the status is ARIA_E_INVALID exactly once; the masked view's
    bytes keep the guard; each good view alone gives the bytes it has in the batch; a second run gives the same bytes."""
    case = RC.scene()
    layout = RC.dense_layout(case.W, case.H)
    h = _handle(aria, work, case.cfg)
    try:
        h.update(_keep := _dev(torch_cuda, work, case.vol))
        got, status = _cast(torch_cuda, work, h, case, layout)
        assert status == ARIA_E_INVALID and h.status() == 0
        assert RC.same_bytes(got, RC.expected(case, layout)) == {}
        for p in RC.PLANES:
            assert (np.frombuffer(got[p][4].tobytes(), np.uint8) == RC.GUARD).all() and not got[p][5].any(), p
        assert (np.frombuffer(got["views"][4:5].tobytes(), np.uint8) == RC.GUARD).all() and got["views"][5].tobytes() == bytes(16)
        again, status = _cast(torch_cuda, work, h, case, layout)
        assert status == ARIA_E_INVALID and RC.same_bytes(again, got) == {}
        for i in range(4):
            one, status = _cast(torch_cuda, work, h, RC.scene_single(i), layout)
            assert status == 0
            for k in RC.PLANES + ("views",):
                assert one[k][0].tobytes() == got[k][i].tobytes(), (i, k)
        # the blocking host form: the same bytes, and ARIA_E_INVALID for the bad view
        c = h.cast(case.ext[1], case.W, case.H)
        want = RC.ref(case)[0][1]
        for k in RC.PLANES + ("view",):
            assert getattr(c, k).tobytes() == getattr(want, k).tobytes(), k
        only = h.cast(case.ext[1], case.W, case.H, planes=1)
        assert only.depth.tobytes() == want.depth.tobytes() and only.normal is None and only.gray is None and only.shade is None
        with pytest.raises(aria.AriaError) as e:
            h.cast(case.ext[5], case.W, case.H)
        assert e.value.status == ARIA_E_INVALID and h.status() == 0
    finally:
        h.close()


@pytest.mark.parametrize("name", ("small_view", "small_tiny", "many_view", "many_tiny"))
def test_padded_layouts_and_null_planes(torch_cuda, work, aria, name):
    """Shape (b): padded pitches and strides on every plane with a guard byte that survives; every combination of one NULL
    plane; no view records. The restatement itself has hits on each branch of rules 7 and 9 (tests/test_ray_host.py)."""
    case = CASES[name]
    layout = RC.padded_layout(case.W, case.H)
    h = _handle(aria, work, case.cfg)
    try:
        h.update(_keep := _dev(torch_cuda, work, case.vol))
        got, status = _cast(torch_cuda, work, h, case, layout)
        assert status == 0 and RC.same_bytes(got, RC.expected(case, layout)) == {}
        for drop in RC.PLANES:
            planes = tuple(p for p in RC.PLANES if p != drop)
            got, status = _cast(torch_cuda, work, h, case, layout, planes)
            assert status == 0 and RC.same_bytes(got, RC.expected(case, layout, planes)) == {}, drop
        got, status = _cast(torch_cuda, work, h, case, layout, views=False)
        want = RC.expected(case, layout)
        want["views"] = RC.guarded(case, layout)["views"]
        assert status == 0 and RC.same_bytes(got, want) == {}
    finally:
        h.close()


def test_chained_volume_update_and_stale_bricks(torch_cuda, work, aria):
    """(d), chained: HipTsdfVolume.integrate_batch_device on TC.scene_frames(), HipVolumeRenderer.from_volume, cast, with no
    host copy of the volume: the bytes of (a). Then six more frames are integrated and the renderer updated again: the cast
    equals the restatement on the new volume (stale brick bits would lose the new surface)."""
    tcfg, _, _ = TC.ref_scene()
    d, im, e = TC.scene_frames()
    vol = aria.HipTsdfVolume(dims=tcfg.dims, voxel=tcfg.voxel, origin=tcfg.origin, trunc=tcfg.trunc, min_depth=tcfg.min_depth,
                             max_depth=tcfg.max_depth, max_weight=tcfg.max_weight, min_weight=tcfg.min_weight, K=tcfg.K,
                             stream=work.cuda_stream)
    h = None
    try:
        def integrate(depths, images, ext):
            keep = [_dev(torch_cuda, work, np.ascontiguousarray(a)) for a in (depths, ext, images)]
            vol.integrate_batch_device(keep[0], TC.W, TC.H, keep[1], len(ext), None, keep[2])
            assert vol.status() == 0
        integrate(d, im, e)
        h = aria.HipVolumeRenderer.from_volume(vol, stream=work.cuda_stream)
        case = RC.scene()
        assert h.ref_config == case.cfg
        layout = RC.dense_layout(case.W, case.H)
        got, status = _cast(torch_cuda, work, h, case, layout)
        assert status == ARIA_E_INVALID and RC.same_bytes(got, RC.expected(case, layout)) == {}
        # a new surface where the first three frames saw free space: a plane at 1.6 m from six new poses (the running mean
        # of a voxel behind it turns negative only after several frames), which sets bits in bricks that had none
        poses = [(0.05 * (-1) ** k, 0.1 * (-1) ** k + 0.02 * k) for k in range(6)]
        r = [TC.render(yaw, x, plane=1.6, sphere=False) for yaw, x in poses]
        d2, im2 = np.stack([a[0] for a in r]), np.stack([a[1] for a in r])
        e2 = np.stack([TC.pose(yaw, x) for yaw, x in poses])
        integrate(d2, im2, e2)
        new_vol, _ = TC.ref_integrated(tcfg, np.concatenate([d, d2]), np.concatenate([e, e2]), np.concatenate([im, im2]))
        assert vol.voxels().tobytes() == new_vol.tobytes()
        new_case = RC.Case("scene_more_frames", new_vol, case.cfg, case.ext, case.mask, case.W, case.H)
        want = RC.expected(new_case, layout)
        assert RC.same_bytes(want, RC.expected(case, layout)) != {}

        def bricks(v):
            f = (v["weight"] >= case.cfg.min_weight) & (v["tsdf"] < 0)
            return f.reshape(f.shape[0] // 8, 8, f.shape[1] // 8, 8, f.shape[2] // 8, 8).any(axis=(1, 3, 5))
        assert (bricks(new_vol) & ~bricks(case.vol)).sum() >= 4       # bricks a stale set of words would skip
        stale, _ = _cast(torch_cuda, work, h, case, layout)          # before the update: the old bricks over the new records
        h.update(vol)
        got, status = _cast(torch_cuda, work, h, case, layout)
        assert status == ARIA_E_INVALID and RC.same_bytes(got, want) == {}
        print("stale bricks differ from the updated cast in", RC.same_bytes(stale, want))
        assert RC.same_bytes(stale, want) != {}                      # else this test no longer shows that update rebuilds the words
    finally:
        if h is not None:
            h.close()
        vol.close()


def test_depth_plane_feeds_the_obstacle_alerter_in_hbm(torch_cuda, work, aria):
    """(e): the depth plane of (a) is handed to HipObstacleAlerter.measure_batch_device as it lies in HBM (pitch and stride
    padded); the result equals alert_ref on the restatement's depth, zone geometry for 80 x 60 as tests/alert_cases.py sets
    it up."""
    case = RC.scene()
    layout = RC.padded_layout(case.W, case.H)
    pitch, stride = layout["depth"]
    assert stride >= pitch * case.H
    h = _handle(aria, work, case.cfg)
    acfg = AC.measure_config(case.W, case.H)
    al = aria.HipObstacleAlerter.from_ref_config(acfg, stream=work.cuda_stream)
    try:
        h.update(_keep := _dev(torch_cuda, work, case.vol))
        n = len(case.ext)
        d_depth = _dev(torch_cuda, work, np.zeros(n * stride, np.float32))       # zeros: the masked view reads as no depth
        d_ext, d_mask = _dev(torch_cuda, work, np.ascontiguousarray(case.ext)), _dev(torch_cuda, work, case.mask)
        h.cast_batch_device(d_ext, n, case.W, case.H, d_depth=d_depth, d_view_mask=d_mask, depth_pitch=pitch, depth_stride=stride)
        d_meas = _dev(torch_cuda, work, np.zeros(n * 64, alert_ref.MEAS_DTYPE))
        al.measure_batch_device(d_depth, stride, pitch, n, d_meas)
        assert h.status() == ARIA_E_INVALID and al.status() == 0
        got = d_meas.cpu().numpy().view(alert_ref.MEAS_DTYPE).reshape(n, 64)
        depth = np.zeros((n, case.H, case.W), np.float32)
        for f, c in enumerate(RC.ref(case)[0]):
            if c is not None:
                depth[f] = c.depth
        want, status, _ = alert_ref.measure(depth, acfg)
        assert status == 0 and got.tobytes() == want.tobytes()
        ok = (want["flags"] & alert_ref.MEAS_OK) != 0
        assert ok[:4].any(axis=1).all() and not ok[4:].any()         # the good views measure something, the blank ones nothing
    finally:
        al.close()
        h.close()


def test_argument_refusals_that_need_a_device(torch_cuda, work, aria):
    torch = torch_cuda
    L = aria.load_library()
    case = RC.small("small")
    h = _handle(aria, work, case.cfg)
    try:
        n, W, H = len(case.ext), case.W, case.H
        d_ext = _dev(torch, work, np.ascontiguousarray(case.ext))
        d_depth = _dev(torch, work, np.full(n * W * H * 4, RC.GUARD, np.uint8))
        def cast(**k):
            return L.aria_ray_cast_batch_device(h._h, k.get("ext", d_ext.data_ptr()), None, k.get("n", n), k.get("w", W), k.get("h", H),
                                                d_depth.data_ptr(), k.get("stride", W * H), k.get("pitch", W), None, 0, 0, None, 0, 0, None,
                                                0, 0, None)
        assert cast() == ARIA_E_INVALID                               # before the first update
        assert L.aria_ray_cast(h._h, case.ext[0].ctypes.data, W, H, None, None, None, None, None) == ARIA_E_INVALID
        assert L.aria_ray_update_from_volume_device(h._h, None) == ARIA_E_INVALID
        h.update(_keep := _dev(torch, work, case.vol))
        for k in (dict(ext=None), dict(n=-1), dict(n=65536), dict(w=-1), dict(h=-1), dict(w=0), dict(h=16385), dict(pitch=W - 1),
                  dict(stride=W * H - 1)):
            assert cast(**k) == ARIA_E_INVALID, k
        assert h.status() == 0 and (d_depth.cpu().numpy() == RC.GUARD).all()      # nothing was enqueued
        assert cast(n=0) == 0 and cast(n=0, ext=None) == 0 and cast() == 0 and h.status() == 0
        assert C.sizeof(type(h.config)) == 96 and h.stream == work.cuda_stream
    finally:
        h.close()


def test_update_holds_the_records_and_refuses_another_geometry(torch_cuda, work, aria):
    """update() keeps the object whose address the handle remembers until the next update or close(), so a tensor handed in
    cannot be freed under the handle; a HipTsdfVolume of another voxel or origin than the renderer's is refused."""
    case = RC.small("small")
    h = _handle(aria, work, case.cfg)
    tcfg = TC.small_config()
    kw = dict(dims=tcfg.dims, trunc=tcfg.trunc, min_depth=tcfg.min_depth, max_depth=tcfg.max_depth, max_weight=tcfg.max_weight,
              min_weight=tcfg.min_weight, K=tcfg.K, stream=work.cuda_stream)
    same = aria.HipTsdfVolume(voxel=tcfg.voxel, origin=tcfg.origin, **kw)
    coarser = aria.HipTsdfVolume(voxel=2 * tcfg.voxel, origin=tcfg.origin, **kw)
    moved = aria.HipTsdfVolume(voxel=tcfg.voxel, origin=(0.0, 0.0, 0.0), **kw)
    try:
        h.update(_dev(torch_cuda, work, case.vol))                   # no other reference to the tensor
        assert h._records is not None
        layout = RC.dense_layout(case.W, case.H)
        got, status = _cast(torch_cuda, work, h, case, layout)
        assert status == 0 and RC.same_bytes(got, RC.expected(case, layout)) == {}
        for other in (coarser, moved):
            with pytest.raises(ValueError):
                h.update(other)
        h.update(same)
        assert h._records is same and h.status() == 0
    finally:
        h.close()
        assert h._records is None
        for v in (same, coarser, moved):
            v.close()

