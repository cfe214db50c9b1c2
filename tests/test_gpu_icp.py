"""Frame-to-model tracking on the MI355X (aria_icp_*, kernels in aria_slam_amd/csrc/icp_track.hip) against its definition, the
NumPy restatement aria_slam_amd/icp_ref.py: the 29 integers of every accumulation, every output pose and every result record
are BITWISE equal. The integer sums are associative, the per-pixel fp32 work rounds every operation once and the fp64 solve
is scalar in a stated order, so a difference is a bug, never a tolerance. The shapes are those of tests/icp_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC   # noqa: E402
from aria_slam_amd import icp_ref as IR   # noqa: E402
from aria_slam_amd import ray_ref as RR   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARIA_E_INVALID = -1


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


def _host(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def _handle(aria, work, cfg):
    return aria.HipDenseTracker.from_ref_config(cfg, stream=work.cuda_stream)


def _layout_kw(lay):
    return dict(depth_pitch=lay["live"][0], depth_stride=lay["live"][1], model_depth_pitch=lay["depth"][0],
                model_depth_stride=lay["depth"][1], normal_pitch=lay["normal"][0], normal_stride=lay["normal"][1])


class Device:
    """The inputs of a batch on the device, kept alive, and the guarded outputs."""

    def __init__(self, torch, work, b, lay, live_fill=None):
        self.torch, self.work, self.b, self.lay = torch, work, b, lay
        self.host = IC.pack(b, lay, live_fill)
        self.dev = {k: _dev(torch, work, v) for k, v in self.host.items()}
        self.mask = None if b.mask is None else _dev(torch, work, b.mask)

    def inputs_intact(self):
        return all(self.dev[k].cpu().numpy().tobytes() == self.host[k].tobytes() for k in self.host)

    def track(self, h, first=0, count=None, poses=True, records=True):
        """One call on frames [first, first + count): (poses, records, status), guarded where nothing is written."""
        n = len(self.b.frames) - first if count is None else count
        hp, hr = IC.guarded_outputs(n)
        dp, dr = _dev(self.torch, self.work, hp), _dev(self.torch, self.work, hr)
        off = lambda key, per: self.dev[key].data_ptr() + per * first   # noqa: E731
        h.track_batch_device(off("live", 4 * self.lay["live"][1]), off("depth", 4 * self.lay["depth"][1]),
                             off("normal", 4 * self.lay["normal"][1]), off("Tm", 96), off("T0", 96), n, self.b.W, self.b.H,
                             d_extrinsics_out=dp if poses else None, d_results=dr if records else None,
                             d_mask=None if self.mask is None else self.mask.data_ptr() + first, **_layout_kw(self.lay))
        status = h.status()
        return _host(dp, hp), _host(dr, hr), status

    def system(self, h, trel, stride):
        n = len(self.b.frames)
        d_trel = _dev(self.torch, self.work, np.ascontiguousarray(trel, np.float64))
        out = np.full((n, IR.N_TERMS), -1, np.int64)
        d_out = _dev(self.torch, self.work, out)
        h.debug_system(self.dev["live"], self.dev["depth"], self.dev["normal"], self.dev["Tm"], d_trel, n, self.b.W, self.b.H, stride,
                       d_out, **_layout_kw(self.lay))
        assert h.status() == 0
        return _host(d_out, out)


def _lay(name):
    f = IC.frame(name)
    return IC.layout(f.W, f.H, padded=name == "pitched")


@pytest.mark.parametrize("name", IC.SINGLES)
def test_debug_system_equals_the_restatements_integers_at_every_level(torch_cuda, work, aria, name):
    f = IC.frame(name)
    cfg = IC.config(f.K)
    d = Device(torch_cuda, work, IC.batch([name]), _lay(name))
    h = _handle(aria, work, cfg)
    try:
        trel = IR.relative(f.Tm, f.T0)
        for stride in (4, 2, 1, 16):
            got = d.system(h, [trel], stride)
            want = IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)
            print("%s stride %d: %d correspondences, differing terms %d" % (name, stride, int(want[28]), int((got[0] != want).sum())))
            assert (got[0] == want).all(), (stride, got[0] - want)
        # the system after the restatement's first step: a Trel that is no longer the guess
        t, trace = IC.ref(name)
        if not trace[0][2].lost:
            trel = IR.advance(trel, trace[0][2].delta)
            assert (d.system(h, [trel], 1)[0] == IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), 1)).all()
        assert d.inputs_intact()
    finally:
        h.close()


def test_partial_tile_lanes_are_masked(torch_cuda, work, aria):
    """`edge`: valid depths in the live map's padding, which only a lane outside W x H can read."""
    cfg, b, lay, trel = IC.edge_case()
    f = b.frames[0]
    d = Device(torch_cuda, work, b, lay, live_fill=IC.EDGE_DEPTH)
    h = _handle(aria, work, cfg)
    try:
        for stride in (4, 2, 1):
            want = IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)
            assert (d.system(h, [trel], stride)[0] == want).all() and want[28] > 0, stride
    finally:
        h.close()


@pytest.mark.parametrize("name", IC.SINGLES)
def test_track_equals_the_restatement_bit_for_bit(torch_cuda, work, aria, name):
    """A batch of one: the pose and the record; the inputs and their padding untouched; a second run gives the same bytes;
    either output may be NULL."""
    f = IC.frame(name)
    cfg = IC.config(f.K)
    b = IC.batch([name])
    d = Device(torch_cuda, work, b, _lay(name))
    h = _handle(aria, work, cfg)
    try:
        poses, recs, status = d.track(h)
        want = IC.expected(b, cfg)
        print(name, recs[0], "pose bytes differ: %d" % int((poses.view(np.uint8) != want[0].view(np.uint8)).sum()))
        assert status == 0 and recs.tobytes() == want[1].tobytes(), (recs, want[1])
        assert poses.tobytes() == want[0].tobytes()
        assert int(recs[0]["valid"]) == (0 if name in IC.LOST else 1) and d.inputs_intact()
        again = d.track(h)
        assert again[0].tobytes() == poses.tobytes() and again[1].tobytes() == recs.tobytes()
        gp, gr = IC.guarded_outputs(1)
        only_p = d.track(h, records=False)
        only_r = d.track(h, poses=False)
        assert only_p[0].tobytes() == poses.tobytes() and only_p[1].tobytes() == gr.tobytes()
        assert only_r[1].tobytes() == recs.tobytes() and only_r[0].tobytes() == gp.tobytes()
    finally:
        h.close()


def test_batch_of_five_at_every_position_split_masked_and_non_finite(torch_cuda, work, aria):
    cfg = IC.config(IC.K)
    lay = IC.layout(IC.W, IC.H, padded=True)
    h = _handle(aria, work, cfg)
    try:
        for shift in range(5):
            b = IC.batch(IC.FIVE[shift:] + IC.FIVE[:shift])
            d = Device(torch_cuda, work, b, lay)
            poses, recs, status = d.track(h)
            want = IC.expected(b, cfg)
            assert status == 0 and recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes(), shift
            if shift == 0:                                            # the same five in two calls
                a, c = d.track(h, 0, 2), d.track(h, 2, 3)
                assert np.concatenate([a[0], c[0]]).tobytes() == poses.tobytes()
                assert np.concatenate([a[1], c[1]]).tobytes() == recs.tobytes() and d.inputs_intact()
        b = IC.batch(IC.FIVE, mask=[1, 0, 1, 1, 0])
        poses, recs, status = Device(torch_cuda, work, b, lay).track(h)
        want = IC.expected(b, cfg)
        assert status == 0 and recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
        gp, gr = IC.guarded_outputs(5)
        for f in (1, 4):
            assert poses[f].tobytes() == gp[f].tobytes() and recs[f:f + 1].tobytes() == gr[f:f + 1].tobytes()
        b = IC.batch(["corner", "corner", "converged"], nan_frame=1)
        d = Device(torch_cuda, work, b, lay)
        poses, recs, status = d.track(h)
        want = IC.expected(b, cfg)
        assert want[2] and status == ARIA_E_INVALID and h.status() == 0       # reported once
        assert recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
        assert recs[1:2].tobytes() == bytes(32) and poses[1].tobytes() == gp[1].tobytes()
    finally:
        h.close()


@pytest.mark.parametrize("levels", IC.LEVELS)
def test_levels(torch_cuda, work, aria, levels):
    b = IC.batch(["corner"])
    cfg = IC.config(IC.K, **levels)
    h = _handle(aria, work, cfg)
    try:
        assert h.ref_config == cfg
        poses, recs, status = Device(torch_cuda, work, b, IC.layout(b.W, b.H)).track(h)
        want = IC.expected(b, cfg)
        assert status == 0 and recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
    finally:
        h.close()


def test_host_form_and_argument_refusals(torch_cuda, work, aria):
    L = aria.load_library()
    f = IC.frame("corner")
    cfg = IC.config(f.K)
    b = IC.batch(["corner", "fused"])
    lay = IC.layout(b.W, b.H)
    d = Device(torch_cuda, work, b, lay)
    h = _handle(aria, work, cfg)
    try:
        t = h.track(f.D, f.M, f.N, f.Tm)
        want = IC.ref("corner")[0]
        assert t.T.tobytes() == want.T.tobytes() and t.result.tobytes() == want.result.tobytes()
        bad = np.array(f.T0)
        bad[3] = np.inf
        with pytest.raises(aria.AriaError) as e:
            h.track(f.D, f.M, f.N, f.Tm, bad)
        assert e.value.status == ARIA_E_INVALID and h.status() == 0
        gp, gr = IC.guarded_outputs(2)
        dp, dr = _dev(torch_cuda, work, gp), _dev(torch_cuda, work, gr)
        W, H = b.W, b.H

        def call(**k):
            p = lambda key: k.get(key, d.dev[key].data_ptr())   # noqa: E731
            return L.aria_icp_track_batch_device(h._h, p("live"), k.get("stride", W * H), k.get("pitch", W), p("depth"), W * H, W,
                                                 p("normal"), k.get("nstride", 3 * W * H), W, p("Tm"), p("T0"), None, k.get("n", 2),
                                                 k.get("w", W), k.get("h", H), dp.data_ptr(), dr.data_ptr())
        for k in (dict(live=None), dict(depth=None), dict(normal=None), dict(Tm=None), dict(T0=None), dict(n=-1), dict(n=4097), dict(w=0),
                  dict(h=16385), dict(w=8192, h=4096), dict(pitch=W - 1), dict(stride=W * H - 1), dict(nstride=3 * W * H - 1)):
            assert call(**k) == ARIA_E_INVALID, k
        assert h.status() == 0 and _host(dp, gp).tobytes() == gp.tobytes() and _host(dr, gr).tobytes() == gr.tobytes()      # nothing enqueued
        assert call(n=0) == 0 and call() == 0 and h.status() == 0
        assert C.sizeof(type(h.config)) == 120 and h.stream == work.cuda_stream
        assert h.algorithmic_bytes(752, 480, 3) == IR.algorithmic_bytes(IR.config(K=f.K), 752, 480, 3)
        out = C.c_void_p()
        for kw in __import__("test_icp_host").BAD:                   # every ValueError of the restatement is ARIA_E_INVALID here
            if len(kw.get("strides", ())) != len(kw.get("iterations", ())):
                continue                                              # two lengths: only the binding can say that
            try:
                c = h._default_config(0, None)
                for key, v in kw.items():
                    if key == "K":
                        c.fx, c.fy, c.cx, c.cy = v
                    elif key in ("strides", "iterations"):
                        if len(v) > 4:
                            c.n_levels = len(v)
                            continue
                        c.n_levels = len(kw["strides"])
                        for l, x in enumerate(v):
                            (c.stride if key == "strides" else c.iterations)[l] = x
                    else:
                        setattr(c, key, v)
            except (TypeError, ValueError, OverflowError):
                continue
            assert L.aria_icp_create(C.byref(c), C.byref(out)) == ARIA_E_INVALID, kw
    finally:
        h.close()


def test_from_renderer_refuses_other_intrinsics(torch_cuda, work, aria):
    _, _, tcfg, rcfg = IC.fused_model()[:4]
    r = aria.HipVolumeRenderer(dims=rcfg.dims, voxel=rcfg.voxel, origin=rcfg.origin, min_weight=rcfg.min_weight, near=rcfg.near,
                               far=rcfg.far, step=rcfg.step, K=rcfg.K, stream=work.cuda_stream)
    try:
        with pytest.raises(ValueError):
            aria.HipDenseTracker.from_renderer(r, (61.0, 60.0, 47.3, 35.3))
        t = aria.HipDenseTracker.from_renderer(r, rcfg.K, stream=work.cuda_stream)
        assert t.ref_config == IC.config(rcfg.K)
        t.close()
    finally:
        r.close()


def test_plain_schedule_of_the_variants_build_equals_the_restatement(aria):
    """One pixel per lane and one atomic set per wave (ARIA_ICP_SCHEDULE=plain, variants build only): the schedule
    tools/icp_rate.py times against gives the same integers, poses and records. As tests/test_gpu_variants.py does, this builds
    libaria_orb_hip_variants.so itself and points a subprocess's binding at it."""
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = aria.build_variants_library()
    e.pop("ARIA_ICP_SCHEDULE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "icp_schedule_check.py")], env=e, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("plain: 0 bytes") == len(IC.SINGLES) and out.stdout.count("shipped: 0 bytes") == len(IC.SINGLES)
    assert "icp schedules agree" in out.stdout


def test_integrate_cast_track_chain_stays_in_hbm_and_equals_the_three_restatements(torch_cuda, work, aria):
    """HipTsdfVolume.integrate_batch_device -> HipVolumeRenderer.cast_batch_device -> HipDenseTracker.track_batch_device on the
    `fused` scene, the model maps never leaving the device: bitwise the chain tsdf_ref -> ray_ref -> icp_ref."""
    M, N, tcfg, rcfg, depths, poses, vol_ref = IC.fused_model()
    f = IC.frame("fused")
    cfg = IC.config(f.K)
    vol = aria.HipTsdfVolume(dims=tcfg.dims, voxel=tcfg.voxel, origin=tcfg.origin, trunc=tcfg.trunc, min_depth=tcfg.min_depth,
                             max_depth=tcfg.max_depth, max_weight=tcfg.max_weight, min_weight=tcfg.min_weight, K=tcfg.K,
                             stream=work.cuda_stream)
    r = t = None
    try:
        keep = [_dev(torch_cuda, work, np.ascontiguousarray(a)) for a in (depths, poses)]
        vol.integrate_batch_device(keep[0], IC.W, IC.H, keep[1], len(poses))
        assert vol.status() == 0
        r = aria.HipVolumeRenderer.from_volume(vol, near=rcfg.near, far=rcfg.far, stream=work.cuda_stream)
        assert r.ref_config == rcfg
        t = aria.HipDenseTracker.from_renderer(r, tcfg.K, stream=work.cuda_stream)
        d_model = _dev(torch_cuda, work, np.zeros(IC.W * IC.H, np.float32))
        d_normal = _dev(torch_cuda, work, np.zeros(3 * IC.W * IC.H, np.float32))
        d_tm, d_live = _dev(torch_cuda, work, np.array(f.Tm)), _dev(torch_cuda, work, f.D)
        gp, gr = IC.guarded_outputs(1)
        dp, dr = _dev(torch_cuda, work, gp), _dev(torch_cuda, work, gr)
        r.cast_batch_device(d_tm, 1, IC.W, IC.H, d_depth=d_model, d_normal=d_normal)
        t.track_batch_device(d_live, d_model, d_normal, d_tm, d_tm, 1, IC.W, IC.H, d_extrinsics_out=dp, d_results=dr)
        assert r.status() == 0 and t.status() == 0
        assert _host(d_model, M).tobytes() == M.tobytes() and _host(d_normal, N).tobytes() == N.tobytes()
        want = IC.ref("fused")[0]
        assert _host(dr, gr)[0].tobytes() == want.result.tobytes() and _host(dp, gp)[0].tobytes() == want.T.tobytes()
        assert int(want.result["valid"]) == 1
    finally:
        for x in (t, r, vol):
            if x is not None:
                x.close()
