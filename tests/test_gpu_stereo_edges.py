"""Sparse stereo on the MI355X at every window, pass, chunk, span, bin, count and key the C-ABI admits: the groups of
tests/stereo_cases.py (edge_groups(), scale_groups()), each as one batch on a handle of its configuration, BITWISE against the
restatement aria_slam_amd/stereo_ref.py -- every aria_stereo_obs record up to kp_stride, the match list and its count, every
aria_stereo_scale. No tolerance anywhere. What each group reaches is asserted without a GPU in tests/test_stereo_edges_host.py.

Layout of every launch: a pitch larger than the width and a padded image stride with 0xA5 in the padding; match_cap larger than
kp_stride; the outputs prefilled with 0x5A, and behind every output, and behind every pair's match list, bytes that must still
be 0x5A afterwards. Every group runs twice on its handle with equal bytes, and pair 0 goes through the blocking host form."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_cases as PC   # noqa: E402
from test_gpu_stereo import _assert_pair_equal, _dev, _padded   # noqa: E402

GUARD = 64                                   # records / rows / counts behind every output


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


def _filled(torch, work, nbytes):
    with torch.cuda.stream(work):
        t = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _upload(torch, work, g):
    w, h, cap = g["width"], g["height"], g["kp_stride"]
    pitch = w + 32
    stride = pitch * h + 64
    il, ir, kl, kr, dl, dr, nl, nr = PC.stack_cases(g["pairs"], cap)
    dev = [_dev(torch, work, _padded(list(il), pitch, stride)), _dev(torch, work, _padded(list(ir), pitch, stride)), stride, w, h, pitch]
    return dev + [_dev(torch, work, a) for a in (kl, dl, nl, kr, dr, nr)] + [cap, len(g["pairs"])]


def _launch(torch, work, st, dev):
    """One aria_stereo_match_batch_device -> (obs (n, cap), matches (n, mcap), counts (n,), status, seconds); asserts the guards."""
    from aria_slam_amd._lib import MATCH_DTYPE, STEREO_OBS_DTYPE
    cap, n = dev[-2], dev[-1]
    mcap = cap + 8
    obs, m, nm = _filled(torch, work, (n * cap + GUARD) * 32), _filled(torch, work, (n * mcap + GUARD) * 12), _filled(torch, work, (n + GUARD) * 4)
    t0 = time.perf_counter()
    st.match_batch_device(*dev, obs, m, nm, match_cap=mcap)
    status = st.status()
    dt = time.perf_counter() - t0
    obs, m, nm = obs.cpu().numpy(), m.cpu().numpy(), nm.cpu().numpy()
    assert (obs[n * cap * 32:] == 0x5A).all() and (m[n * mcap * 12:] == 0x5A).all() and (nm[n * 4:] == 0x5A).all(), "a guard was written"
    return (obs[:n * cap * 32].view(STEREO_OBS_DTYPE).reshape(n, cap), m[:n * mcap * 12].view(MATCH_DTYPE).reshape(n, mcap),
            nm[:n * 4].view(np.int32), status, dt)


def _check_group(g, obs, m, nm):
    for p, c in enumerate(g["pairs"]):
        want_obs, want_m = PC.edge_restatement(g["name"], p)
        _assert_pair_equal(c["name"], obs[p], m[p], nm[p], want_obs, want_m)
        assert (m[p][nm[p]:].view(np.uint8) == 0x5A).all(), (c["name"], "rows beyond the count were written")
        for i, e in enumerate(c["expect"]):
            assert obs[p][i]["right_idx"] == (e[0] if e else -1), (c["name"], i)


@pytest.mark.parametrize("name", [g["name"] for g in PC.edge_groups()])
def test_match_group_equals_the_restatement(aria, torch_cuda, work, name):
    torch = torch_cuda
    g = PC.edge_group(name)
    dev = _upload(torch, work, g)
    st = aria.HipStereoMatcher(stream=work.cuda_stream, **g["cfg"])
    try:
        obs, m, nm, status, dt = _launch(torch, work, st, dev)
        assert status == 0
        _check_group(g, obs, m, nm)
        obs2, m2, nm2, status, dt2 = _launch(torch, work, st, dev)
        assert status == 0 and obs2.tobytes() == obs.tobytes() and m2.tobytes() == m.tobytes() and nm2.tobytes() == nm.tobytes()
        print("%s: %d pairs, kp_stride %d, %d bytes of dynamic LDS, %.1f ms and %.1f ms" %
              (name, len(g["pairs"]), g["kp_stride"], PC.match_lds_bytes(g), 1e3 * dt, 1e3 * dt2))
        c = g["pairs"][0]                                                       # the blocking host form, on a strided view
        pad = np.zeros((2, g["height"], g["width"] + 8), np.uint8)
        pad[0, :, :g["width"]], pad[1, :, :g["width"]] = c["img_l"], c["img_r"]
        o, mm = st.match(pad[0, :, :g["width"]], pad[1, :, :g["width"]], (c["kp_l"], c["desc_l"]), (c["kp_r"], c["desc_r"]))
        want_obs, want_m = PC.edge_restatement(name, 0)
        assert o.tobytes() == want_obs.tobytes() and mm.tobytes() == want_m.tobytes()
    finally:
        st.close()


def test_one_handle_through_shapes_that_shrink_and_grow(aria, torch_cuda, work):
    """4096 rows, then 64, then 480 on one handle: nothing of an earlier launch's LDS layout or staging survives into the next."""
    torch = torch_cuda
    groups = [PC.edge_group(n) for n in ("rows H=4096", "counts", "rows H=480", "rows H=4096")]
    assert [g["height"] for g in groups] == [4096, 64, 480, 4096] and all(g["cfg"] == PC.CFG_ROWS for g in groups)
    st = aria.HipStereoMatcher(stream=work.cuda_stream, **PC.CFG_ROWS)
    try:
        for g in groups:
            obs, m, nm, status, _ = _launch(torch, work, st, _upload(torch, work, g))
            assert status == 0
            _check_group(g, obs, m, nm)
            c = g["pairs"][-1]
            o, mm = st.match(c["img_l"], c["img_r"], (c["kp_l"], c["desc_l"]), (c["kp_r"], c["desc_r"]))
            want_obs, want_m = PC.edge_restatement(g["name"], len(g["pairs"]) - 1)
            assert o.tobytes() == want_obs.tobytes() and mm.tobytes() == want_m.tobytes()
    finally:
        st.close()


@pytest.mark.parametrize("g", PC.scale_groups(), ids=lambda g: g["name"])
def test_scale_group_equals_the_restatement(aria, torch_cuda, work, g):
    from aria_slam_amd._lib import STEREO_SCALE_DTYPE
    torch = torch_cuda
    pose, mask, m, nm, oq, nq, ot, nt = PC.scale_arrays(g)
    n, cap = len(pose), g["match_cap"]
    d = [_dev(torch, work, a) for a in (pose, mask, m, nm, oq, nq, ot, nt)]
    st = aria.HipStereoMatcher(stream=work.cuda_stream, **g["cfg"])
    try:
        runs = []
        for _ in range(2):
            out = _filled(torch, work, (n + GUARD) * 16)
            t0 = time.perf_counter()
            st.scale_batch_device(d[0], d[1] if g["with_mask"] else None, d[2], d[3], cap, d[4], d[5], d[6], d[7], g["kp_stride"], n, out,
                                  query_is_first=g["query_is_first"])
            assert st.status() == 0
            dt = time.perf_counter() - t0
            out = out.cpu().numpy()
            assert (out[n * 16:] == 0x5A).all(), "the guard was written"
            runs.append(out[:n * 16].view(STEREO_SCALE_DTYPE))
        print("%s: %d records, match_cap %d, %d bytes of dynamic LDS, %.1f ms" % (g["name"], n, cap, 8 * cap, 1e3 * dt))
        assert runs[0].tobytes() == runs[1].tobytes()
        for p, r in enumerate(g["records"]):
            want = PC.scale_restatement(g, p)
            assert runs[0][p].tobytes() == want.tobytes(), (r["name"], runs[0][p], want)
            assert (float(runs[0][p]["scale"]), int(runs[0][p]["n_used"]), int(runs[0][p]["valid"])) == r["expect"], r["name"]
        for p in (0, len(g["records"]) - 1):                                    # the blocking host form
            k = nm[p]
            single = st.scale(pose[p], m[p, :k], oq[p, :k], ot[p, :k], mask=mask[p, :k] if g["with_mask"] else None,
                              query_is_first=g["query_is_first"])
            assert single.tobytes() == runs[0][p].tobytes(), g["records"][p]["name"]
    finally:
        st.close()
