"""The point map's many-round paths on the MI355X (kernels in aria_slam_amd/csrc/map_triangulate.hip): an append whose pair
scan takes three rounds of 1024 with the carry between them, a capacity verdict that falls in a later round on a map that
is not empty, reserve() copying live points, filters over more than 256 blocks (k_map_stats' strided loop) and more than
1024 (k_map_fscan's carry), a small map in a large arena, reserve() out of the swapped arena, windowed reads, the device
pointer, the blocking form's own growth, and non-finite keypoints.

The float fields are held to the extended run of the restatement by test_gpu_map.hold (bounds and GAP in that module's
docstring); everything else is compared bitwise, with another run of the device or with map_ref's filters."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases   # noqa: E402
from map_cases import SCALE_BASE as BASE, SCALE_CAP as CAP, SCALE_PAIRS as P_   # noqa: E402
from test_gpu_map import _batch, _views, hold   # noqa: E402

pytestmark = pytest.mark.gpu

ARIA_E_INVALID, ARIA_E_OUTPUT_TOO_SMALL = -1, -5
BIG = (1 << 20) + 40 * 1024          # 1064 filter blocks of 1024 points


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _device(torch, b):
    """scale_batch's host arrays as the device blocks _batch takes."""
    dev = torch.device("cuda", 0)
    t = lambda x, n: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1, n).copy()).to(dev)
    n = torch.from_numpy(b["n"]).to(dev)
    d = dict(kq=t(b["kq"], 24), kt=t(b["kt"], 24), mm=t(b["mm"], 12), nq=n, nt=n, nm=n, ext=torch.from_numpy(b["ext"]).to(dev))
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def scale(aria, torch_cuda):
    """The 2600-pair batch on the device, the restatement's kept matches per rig, its count per pair, and the map and
    `added` of one launch into an empty handle."""
    torch = torch_cuda
    b = map_cases.scale_batch()
    d = _device(torch, b)
    want = np.zeros(P_, np.int64)
    rigs = []
    for k in range(4):
        pair, match, i1, i2 = map_cases.scale_rig(k)[:4]
        kept = np.flatnonzero(map_cases.ref_runs("scale%d" % k)[1]["keep"])
        rigs.append((kept, pair[kept], match[kept], i1[kept], i2[kept]))
        want += np.bincount(pair[kept], minlength=P_)
    mp = aria.HipMapper()
    try:
        added = torch.full((P_,), -1, dtype=torch.int32, device=d["nm"].device)
        torch.cuda.synchronize()
        _batch(mp, d, CAP, 0, P_, BASE, added)
        mp.check()
        got, added = mp.read(), added.cpu().numpy()
    finally:
        mp.close()
    return dict(host=b, dev=d, want=want, rigs=rigs, map=got, added=added)


def _append(torch, mp, d, lo, hi):
    """Pairs [lo, hi) of the batch in one launch; returns `added` of those pairs (-1 where the launch wrote nothing)."""
    added = torch.full((P_,), -1, dtype=torch.int32, device=d["nm"].device)
    torch.cuda.synchronize()
    _batch(mp, d, CAP, lo, hi, BASE, added)
    return added


def test_append_over_three_scan_rounds(aria, torch_cuda, scale):
    torch = torch_cuda
    got, want = scale["map"], scale["want"]
    assert np.array_equal(scale["added"], want)                          # per pair, the restatement's count
    assert (want[scale["host"]["n"] < 8] == 0).all() and (want[list(map_cases.SCALE_FULL)] > 0).all()
    assert len(got) == want.sum() > 15000
    assert np.array_equal(got["id"], np.arange(len(got)))                # no gap at pairs 1023/1024 or 2047/2048
    assert np.array_equal(got["pair"], BASE + np.repeat(np.arange(P_), want))
    assert (got["gray"] == 127).all()
    for k, (kept, pair, match, i1, i2) in enumerate(scale["rigs"]):
        g = got[(got["pair"] - BASE) % 4 == k]
        assert np.array_equal(g["pair"], BASE + pair) and np.array_equal(g["match"], match)     # the kept set: identical
        assert np.array_equal(g["idx1"], i1) and np.array_equal(g["idx2"], i2) and (i1 != i2).any()
        hold("scale%d" % k, g, kept)
    mp = aria.HipMapper()
    try:
        # split so that the round boundary falls inside, at the end of, and before a call
        added = torch.full((P_,), -1, dtype=torch.int32, device=scale["dev"]["nm"].device)
        torch.cuda.synchronize()
        for lo, hi in ((0, 1024), (1024, 1025), (1025, P_)):
            _batch(mp, scale["dev"], CAP, lo, hi, BASE, added)
        mp.check()
        assert mp.read().tobytes() == got.tobytes() and np.array_equal(added.cpu().numpy(), want)
        # an out-of-range match index in a pair of the second round and in one of the third
        bad = (1500, 2300)
        host = dict(scale["host"], mm=scale["host"]["mm"].copy())
        host["mm"]["train_idx"][1500, 11] = CAP                            # == nt
        host["mm"]["query_idx"][2300, 23] = -1
        d2 = _device(torch, host)
        mp.clear()
        added = _append(torch, mp, d2, 0, P_)
        assert mp.status() == ARIA_E_INVALID
        assert mp.status() == 0                                            # reported once
        a = added.cpu().numpy()
        assert (a[list(bad)] == 0).all() and np.array_equal(np.delete(a, bad), np.delete(want, bad))
        clean = got[~np.isin(got["pair"], BASE + np.array(bad))].copy()
        clean["id"] = np.arange(len(clean))
        assert mp.read().tobytes() == clean.tobytes()
    finally:
        mp.close()


def test_capacity_verdict_in_a_later_round_then_reserve_with_live_points(aria, torch_cuda, scale):
    torch = torch_cuda
    got, want, d = scale["map"], scale["want"], scale["dev"]
    cut = 1700
    assert want[cut] > 0
    first = int(want[:200].sum())
    fits = int(want[:cut].sum())
    mp = aria.HipMapper(capacity=fits + int(want[cut]) - 1)
    try:
        added = _append(torch, mp, d, 0, 200)
        mp.check()
        assert mp.size() == first > 0 and np.array_equal(added.cpu().numpy()[:200], want[:200])
        # pairs 200..2599: the pair that does not fit is position 1500 of this launch, in the scan's second round
        added = _append(torch, mp, d, 200, P_)
        assert mp.status() == ARIA_E_OUTPUT_TOO_SMALL
        assert mp.status() == 0
        a = added.cpu().numpy()
        assert np.array_equal(a[200:cut], want[200:cut]) and (a[cut:] == 0).all() and (a[:200] == -1).all()
        assert (want[cut + 1:] > 0).any() and 0 < want[cut + 1:][want[cut + 1:] > 0].min() < want[cut]   # some would fit alone
        assert mp.size() == fits and mp.points_needed() == want.sum()
        assert mp.read().tobytes() == got[:fits].tobytes()
        cap0 = mp.capacity
        mp.reserve(mp.points_needed())                                     # copies the live points
        assert mp.capacity == want.sum() > cap0 and mp.size() == fits
        assert mp.read().tobytes() == got[:fits].tobytes()
        added = _append(torch, mp, d, cut, P_)
        mp.check()
        assert np.array_equal(added.cpu().numpy()[cut:], want[cut:])
        assert mp.read().tobytes() == got.tobytes()
    finally:
        mp.close()


def _filter_pairs():
    """The three pairs of test_filters_match_map_ref: 400 points at 1-4 units and 6 planted at 40-48."""
    from aria_slam_amd import map_ref as M
    from aria_slam_amd._lib import KP_DTYPE
    E1, E2 = _views(2)
    out = []
    for k in range(3):
        kq, kt, m, _, _ = M.synth_scene(90 + k, 400, E1, E2, depth=(1.0, 4.0))
        far, fkt, fm, _, _ = M.synth_scene(95 + k, 6, E1, E2, depth=(40.0, 48.0), noise_px=0.0)
        fm = fm.copy()
        fm["query_idx"] += 400
        fm["train_idx"] += 400
        out.append((np.concatenate([kq, far]).astype(KP_DTYPE), np.concatenate([kt, fkt]).astype(KP_DTYPE),
                    np.concatenate([m, fm]), E1, E2))
    return out


@pytest.fixture(scope="module")
def big(aria):
    """One handle of BIG points for both large-arena tests: two arenas of 78 MB."""
    mp = aria.HipMapper(capacity=BIG)
    yield mp
    mp.close()


def test_filters_of_a_small_map_in_a_large_arena(aria, big):
    """About 1200 points in 1064 filter blocks: the empty blocks contribute nothing to the sums, and the chunked block
    scan carries across them."""
    small = aria.HipMapper()
    try:
        big.clear()
        for k, pair in enumerate(_filter_pairs()):
            assert big.triangulate(*pair, pair_id=k) == small.triangulate(*pair, pair_id=k)
        n0 = small.size()
        assert n0 > 1000 and big.read().tobytes() == small.read().tobytes()
        big.filter_outliers()
        small.filter_outliers()
        big.check()
        n1 = small.size()
        assert 0 < n1 < n0 and big.read().tobytes() == small.read().tobytes()
        big.filter_distance(3.0)
        small.filter_distance(3.0)
        big.check()
        assert 0 < small.size() < n1 and big.read().tobytes() == small.read().tobytes()
        assert big.capacity == BIG
    finally:
        small.close()


FILL_PAIRS, FILL_CAP = 128, 1024
FILL_DEPTH = (1.0, 3.2)              # units from view 1: filter_distance(3.0) then removes less than half
FILL_FAR = (3, 20, 45, 60, 100)         # pairs of the block whose last 8 matches are planted at 40-48 units


def _fill_block():
    """One block of 128 pairs x 1024 matches on rig 2, 3 % of them random-pixel outliers so that the pairs' kept counts differ
    and the filter blocks do not line up with the pairs: host arrays for _device."""
    from aria_slam_amd import map_ref as M
    from aria_slam_amd._lib import MATCH_DTYPE
    E1, E2 = _views(2)
    kq, kt, _, _, _ = M.synth_scene(400, FILL_PAIRS * FILL_CAP, E1, E2, outlier_frac=0.03, depth=FILL_DEPTH)
    kq, kt = kq.reshape(FILL_PAIRS, FILL_CAP).copy(), kt.reshape(FILL_PAIRS, FILL_CAP).copy()
    for j, p in enumerate(FILL_FAR):
        a, b, _, _, _ = M.synth_scene(410 + j, 8, E1, E2, depth=(40.0, 48.0), noise_px=0.0)
        kq[p, -8:], kt[p, -8:] = a, b
    mm = np.zeros((FILL_PAIRS, FILL_CAP), MATCH_DTYPE)
    mm["query_idx"] = mm["train_idx"] = np.arange(FILL_CAP)
    ext = np.tile(np.concatenate([E1.reshape(-1), E2.reshape(-1)]), (FILL_PAIRS, 1))
    return dict(kq=kq, kt=kt, mm=mm, n=np.full(FILL_PAIRS, FILL_CAP, np.int32), ext=ext)


def _hip_runtime():
    """The HIP runtime this process already has mapped."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime mapped")


def _windows(aria, mp, full, across=None):
    """read(first, count) at 0, in the middle or across record `across`, ending at the size, and empty; one past the size is
    refused."""
    size = len(full)
    assert mp.size() == size > 2000 and (across is None or across + 500 < size)
    mid = size // 2 if across is None else across
    for first, count in ((0, 1000), (mid - 500, 1000), (size - 777, 777), (size, 0), (5, 0)):
        assert mp.read(first, count).tobytes() == full[first:first + count].tobytes(), (first, count)
    with pytest.raises(aria.AriaError) as e:
        mp.read(size - 9, 10)                                # first + count == size + 1
    assert e.value.status == ARIA_E_INVALID


def test_filters_of_a_full_large_arena(aria, torch_cuda, big):
    """More than 1,050,000 points: k_map_stats sums more than 256 block partials, k_map_fscan scans more than 1024 block
    counts. The fill is not re-derived (the scan tests cover the append); both filters are, bitwise, from the map read
    before them. Then the paths that follow a filter's arena swap."""
    from aria_slam_amd import map_ref as M
    torch = torch_cuda
    EXT = map_cases.EXT
    d = _device(torch, _fill_block())
    big.clear()
    for call in range(9):                                    # whole pairs append while they fit: the last call is cut
        _batch(big, d, FILL_CAP, 0, FILL_PAIRS, base=call * FILL_PAIRS)
        assert big.status() == (ARIA_E_OUTPUT_TOO_SMALL if call == 8 else 0)
    before = big.read()
    n0 = len(before)
    assert 1050000 < n0 <= BIG and np.array_equal(before["id"], np.arange(n0))
    _windows(aria, big, before, across=1024 * 1024)
    # the conditions under which this input tests what it is meant to, from `before` in extended precision
    X = before["X"].astype(EXT)
    mean = X.sum(0) / n0
    r = np.sqrt(((X - mean) ** 2).sum(1))
    lim = 3 * np.sqrt((r * r).sum() / n0)
    gone = np.flatnonzero(r > lim) // 1024
    assert (gone < 256).any() and ((gone >= 256) & (gone < 1024)).any() and (gone >= 1024).any()
    assert 100 <= len(gone) <= n0 // 2
    assert (np.abs(r - lim) / lim).min() >= 1e-9             # a last-bit difference in mean or sd decides no point
    want = M.filter_outliers(before)
    assert len(want) == n0 - len(gone)
    big.filter_outliers()
    big.check()
    got = big.read()
    assert got.tobytes() == want.tobytes()
    X = got["X"].astype(EXT)
    r = np.sqrt((X * X).sum(1))
    gone = np.flatnonzero(r > 3.0) // 1024
    assert (gone < 256).any() and ((gone >= 256) & (gone < 1024)).any() and (gone >= 1024).any()
    assert 100 <= len(gone) <= len(got) // 2 and (np.abs(r - 3.0) / 3.0).min() >= 1e-9
    want = M.filter_distance(got, 3.0)
    assert len(want) == len(got) - len(gone)
    big.filter_distance(3.0)
    big.check()
    assert big.read().tobytes() == want.tobytes()
    # ids continue from the next id before the filters, not from the size
    kq, kt, m, E1, E2 = _filter_pairs()[0]
    n = big.triangulate(kq, kt, m, E1, E2, pair_id=7)
    size = big.size()
    assert n > 300 and size == len(want) + n and big.capacity == BIG
    full = big.read()
    assert full[:len(want)].tobytes() == want.tobytes() and np.array_equal(full["id"][len(want):], n0 + np.arange(n))
    # reserve() copies out of the arena the filters swapped in
    big.reserve(BIG + 1024)
    assert big.capacity == BIG + 1024 and big.size() == size and big.read().tobytes() == full.tobytes()
    _windows(aria, big, full)
    # the device pointer: size() records
    ptr = big.device_points()
    assert ptr
    out = np.zeros(size, full.dtype)
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    assert out.tobytes() == full.tobytes()


def test_the_blocking_form_grows_the_arena_itself(aria):
    from aria_slam_amd import map_ref as M
    E1, E2 = _views(1)
    pairs = [M.synth_scene(500 + k, 220, E1, E2, depth=(1.0, 8.0))[:3] for k in range(6)]
    mp = aria.HipMapper(capacity=300)
    ref = aria.HipMapper()
    try:
        caps = []
        for k, (kq, kt, m) in enumerate(pairs):
            n = mp.triangulate(kq, kt, m, E1, E2, pair_id=k)
            assert n == ref.triangulate(kq, kt, m, E1, E2, pair_id=k) and 150 < n <= 220
            assert mp.status() == 0 and mp.capacity >= mp.size() == ref.size()
            caps.append(mp.capacity)
        assert caps[0] == 300 and len(set(caps)) >= 3            # grew at least twice, each time with live points
        got = mp.read()
        assert got.tobytes() == ref.read().tobytes() and np.array_equal(got["id"], np.arange(len(got)))
        assert mp.points_needed() == len(got)
    finally:
        mp.close()
        ref.close()


def test_non_finite_keypoints_are_rejected(aria):
    """NaN, +Inf, -Inf and 3e38 in a keypoint coordinate: the match is dropped without an error, and nothing else moves --
    the map is that of the same pair with those matches switched off by the candidate mask."""
    kq, kt, m, E1, E2, bad = map_cases.nonfinite_pair()
    img = ((np.arange(480 * 752) * 3) % 256).astype(np.uint8).reshape(480, 752)
    mask = np.ones(len(m), np.uint8)
    mask[bad] = 0
    mp = aria.HipMapper()
    try:
        n = mp.triangulate(kq, kt, m, E1, E2, image=img, pair_id=4)
        assert mp.status() == 0
        got = mp.read()
        assert n == len(got) > 400 and not np.isin(bad, got["match"]).any()
        assert np.isfinite(got["X"]).all() and np.isfinite(got["err"]).all() and np.isfinite(got["quality"]).all()
        mp.clear()
        assert mp.triangulate(kq, kt, m, E1, E2, image=img, mask=mask, pair_id=4) == n
        assert mp.read().tobytes() == got.tobytes()
    finally:
        mp.close()
