"""Guided matching on the MI355X at every limit and size the C-ABI admits: the groups of tests/proj_cases.py, edge_groups(), each
on a handle of its own configuration, through aria_proj_search_batch_device between guard bytes. Every byte of obs, corr, pairs
and ncorr equals the restatement (aria_slam_amd/proj_ref.py) and the answers written down from the construction
(tests/test_proj_edges_host.py holds the two to each other and asserts what the groups reach). These are the launches
tests/test_gpu_proj.py never makes: kp_stride = n = 8192, land_cap = count = 2^20, a grid of 16384 cells (65 KiB of dynamic LDS
in k_proj_bin), of one cell, one row and one column, a span of 8192 entries under the 16-lane walk, windows of the whole grid,
every end of the configuration's ranges, and one handle called with shapes that shrink and grow again."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_cases as PC   # noqa: E402
import test_gpu_proj as G   # noqa: E402
from test_gpu_proj import torch_cuda, work   # noqa: E402,F401  (fixtures)

INVALID = G.INVALID


def _matcher(aria, work, g):
    from aria_slam_amd import proj_ref as R
    c = dict(R.DEFAULTS, **g["cfg"])
    return aria.HipProjectionMatcher(K=c["K"], min_depth=c["min_depth"], radius_px=c["radius_px"], ratio=c["ratio"], th_hamming=c["th_hamming"],
                                     max_octave_diff=c["max_octave_diff"], stream=work.cuda_stream)


def _run(torch, work, pm, g, frames, ns=None):
    """One call of aria_proj_search_batch_device: the given frames of group g as a batch. ns overrides the counts d_n says."""
    arrays = [PC.edge_frame_arrays(g, f) for f in frames]
    return G._search(torch, work, pm, [f["pose"] for f in frames], [a[0] for a in arrays], [a[1] for a in arrays],
                     [f["n"] for f in frames] if ns is None else ns, g["kp_stride"], g["width"], g["height"], g["landmarks"],
                     [(f["first"], f["count"]) for f in frames], g["land_cap"])


def _check(g, frames, out):
    """Every frame of the batch against the restatement AND the written answers."""
    obs, corr, pairs, ncorr, _ = out
    for j, f in enumerate(frames):
        want, written = PC.edge_restatement(g, f), PC.edge_expected(g, f)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, written)), f["name"]
        G._assert_frame("%s / %s" % (g["name"], f["name"]), obs[j], corr[j], pairs[j], ncorr[j], *want)
    assert np.isfinite(obs["u"]).all() and np.isfinite(obs["v"]).all()


def _bytes(out):
    return [x.tobytes() for x in out[:4]]


@pytest.mark.parametrize("name", [g["name"] for g in PC.edge_groups()])
def test_each_group_as_its_own_batch_on_a_fresh_handle(aria, torch_cuda, work, name):
    g = PC.edge_group(name)
    t0 = time.perf_counter()
    pm = _matcher(aria, work, g)
    try:
        out = _run(torch_cuda, work, pm, g, g["frames"])
        again = pm.status()
    finally:
        pm.close()
    assert out[4] == 0 and again == 0
    _check(g, g["frames"], out)
    print("%s: %d frame(s), %d matched, %.2f s" % (name, len(g["frames"]), int(out[3].sum()), time.perf_counter() - t0))


GRID_ORDER = ["grid 4096x4096", "grid 32x32", "grid 33x31", "grid 4096x1", "grid 1x4096", "grid 4096x4096"]
GRID_FRAMES = [1, 3, 1, 2, 2, 1]


def test_grids_on_one_handle_shrinking_and_growing_in_both_orders(aria, torch_cuda, work):
    """One handle, six calls whose cell count goes 16384, 1, 2, 128, 128, 16384, whose n_frames goes 1, 3, 1, 2, 2, 1 and whose
    kp_stride goes 13, 7, 6, 8, 8, 13: the grow-only workspace is addressed with the strides of the call. Then the same calls
    in reverse on a second handle: the bytes of a call do not depend on what the handle served before."""
    calls = list(zip(GRID_ORDER, GRID_FRAMES))
    assert len({PC.edge_group(n)["kp_stride"] for n, _ in calls}) >= 4
    seen = {}
    for order in (calls, calls[::-1]):
        g0 = PC.edge_group(order[0][0])
        pm = _matcher(aria, work, g0)
        try:
            for j, (name, reps) in enumerate(order):
                g = PC.edge_group(name)
                assert g["cfg"]["K"] == g0["cfg"]["K"]
                frames = g["frames"] * reps
                out = _run(torch_cuda, work, pm, g, frames)
                assert out[4] == 0
                _check(g, frames, out)
                key = (name, reps, j if order is calls else len(calls) - 1 - j)
                if key in seen:
                    assert seen[key] == _bytes(out), key
                seen[key] = _bytes(out)
        finally:
            pm.close()
    assert len(seen) == len(calls)


@pytest.mark.parametrize("name", ["index_bits", "spans one cell", "spans whole grid"])
def test_three_equal_frames_then_beside_an_invalid_one(aria, torch_cuda, work, name):
    """The first frame of the group three times in one batch: three equal rows. Then the frame, an invalid frame whose d_n is
    kp_stride + 1 (8193 for the first two groups) and the frame again: the invalid one leaves records that are not visible,
    a count of 0 and corr and pairs untouched; its neighbours are unaffected; the status is reported once."""
    g = PC.edge_group(name)
    f = g["frames"][0]
    pm = _matcher(aria, work, g)
    try:
        out = _run(torch_cuda, work, pm, g, [f, f, f])
        assert out[4] == 0
        _check(g, [f, f, f], out)
        for x in out[:4]:
            assert x[0].tobytes() == x[1].tobytes() == x[2].tobytes()
        bad = _run(torch_cuda, work, pm, g, [f, f, f], ns=[f["n"], g["kp_stride"] + 1, f["n"]])
        again = pm.status()
    finally:
        pm.close()
    assert bad[4] == INVALID and again == 0
    obs, corr, pairs, ncorr, _ = bad
    _check(g, [f], (obs[:1], corr[:1], pairs[:1], ncorr[:1], 0))
    _check(g, [f], (obs[2:], corr[2:], pairs[2:], ncorr[2:], 0))
    from aria_slam_amd import proj_ref as R
    assert obs[1].tobytes() == R.not_visible_obs(g["land_cap"]).tobytes() and ncorr[1] == 0
    assert (corr[1].view(np.uint8) == 0x5A).all() and (pairs[1].view(np.uint8) == 0x5A).all()


@pytest.mark.parametrize("name", ["index_bits", "claim_bits"])
def test_blocking_host_form_at_the_limits(aria, torch_cuda, work, name):
    """aria_proj_search through HipProjectionMatcher.search at n = 8192 (index_bits, frame A: its range is the whole array) and
    at n_landmarks = 2^20 (claim_bits, the written live list)."""
    g = PC.edge_group(name)
    f = g["frames"][0]
    assert f["first"] == 0 and f["count"] == len(g["landmarks"]) and (f["n"] == 8192 or f["count"] == 1 << 20)
    pm = _matcher(aria, work, g)
    try:
        obs, corr, pairs = pm.search(f["pose"], f["kp"], f["desc"], g["landmarks"], g["width"], g["height"])
        assert pm.status() == 0
    finally:
        pm.close()
    want_obs, want_corr, want_pairs = PC.edge_expected(g, f)
    assert obs.tobytes() == want_obs[:f["count"]].tobytes() and corr.tobytes() == want_corr.tobytes() and pairs.tobytes() == want_pairs.tobytes()


@pytest.mark.parametrize("name", ["claim_bits", "spans one cell"])
def test_run_to_run_repeat_has_equal_bytes(aria, torch_cuda, work, name):
    g = PC.edge_group(name)
    runs = []
    for _ in range(2):
        pm = _matcher(aria, work, g)
        try:
            runs.append(_run(torch_cuda, work, pm, g, g["frames"]))
        finally:
            pm.close()
    assert runs[0][4] == runs[1][4] == 0 and _bytes(runs[0]) == _bytes(runs[1])
