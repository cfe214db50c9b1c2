"""Sparse stereo at every window, pass, chunk, span, bin, count and key the C-ABI admits (tests/stereo_cases.py, edge_groups() and
scale_groups()), without a GPU: the restatement aria_slam_amd/stereo_ref.py against the answers written down from each
construction, and a census asserting that the groups reach what they claim to reach, computed from the restatement and the
documented geometry of csrc/stereo_match.hip alone (16 lanes per left keypoint, a shift per lane and pass; 64 candidates per
step of the search; ceil(H / 256) rows per thread of the row scan; two 256-bin histograms of the SAD; eight radix passes over
the scale keys; 4 bytes of LDS per row and 16 per keypoint). A group that stops reaching its branch fails here.

CPU time of the restatement over all groups: 3 s, the slowest group `span 8192` (570 x 8192 candidate tests) 1.2 s, then
`counts nL=8192` 0.5 s; every other group below 0.1 s."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_cases as PC   # noqa: E402
from aria_slam_amd import stereo_ref as R   # noqa: E402

_F = np.float32
GROUPS = {g["name"]: g for g in PC.edge_groups()}


def _pairs():
    return [pytest.param(g["name"], p, id="%s / %s" % (g["name"], c["name"])) for g in PC.edge_groups() for p, c in enumerate(g["pairs"])]


@pytest.mark.parametrize("name,p", _pairs())
def test_restatement_equals_the_written_answers(name, p):
    g = GROUPS[name]
    c = g["pairs"][p]
    obs, m = PC.edge_restatement(name, p)
    assert len(obs) == len(c["expect"]) == len(c["kp_l"])
    for i, e in enumerate(c["expect"]):
        assert int(obs["right_idx"][i]) == (e[0] if e else -1), (c["name"], i, e, obs[i])
        if e and e[1] is not None:
            d = float(obs["disparity"][i])
            assert (abs(d - e[1]) <= 0.5) if e[1] >= 1 else d == float(R.MIN_DISPARITY_CLAMP), (c["name"], i, e, d)
    kept = [i for i, e in enumerate(c["expect"]) if e]
    assert m["query_idx"].tolist() == kept and m["train_idx"].tolist() == [c["expect"][i][0] for i in kept]
    assert np.isfinite(np.stack([obs[f] for f in ("u_right", "disparity", "depth", "X", "Y")])).all()


@pytest.mark.parametrize("g", PC.scale_groups(), ids=lambda g: g["name"])
def test_scale_restatement_equals_the_written_answers(g):
    for p, r in enumerate(g["records"]):
        got = PC.scale_restatement(g, p)
        assert (float(got["scale"]), int(got["n_used"]), int(got["valid"])) == r["expect"], (r["name"], got, r["expect"])


# ---- census ----------------------------------------------------------------------------------------------------------------------
def _trace(g, c):
    """Per left keypoint whose slide ran: (i, j, SAD array, best index)."""
    cfg = R._config(g["cfg"])
    w, L = int(cfg["sad_half_window"]), int(cfg["sad_slide"])
    best, dist = R.best_candidates(c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **g["cfg"])
    out = []
    for i in range(len(c["kp_l"])):
        j = int(best[i])
        if j < 0 or dist[i] >= cfg["th_hamming"]:
            continue
        ul, vl, ur = (int(np.rint(v)) for v in (c["kp_l"]["x"][i], c["kp_l"]["y"][i], c["kp_r"]["x"][j]))
        sad = R.sad_slide(c["img_l"], c["img_r"], ul, vl, ur, w, L)
        if sad is not None:
            out.append((i, j, sad, int(np.argmin(sad))))
    return out


def _prefilter_sads(g, c):
    """The SADs that reach the median: the restatement with a median factor nothing exceeds (inf * 0 is a NaN, which nothing
    exceeds either)."""
    with np.errstate(invalid="ignore"):
        obs, _ = R.stereo_match_ref(c["img_l"], c["img_r"], c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **dict(g["cfg"], median_factor=np.inf))
    return obs["sad"][obs["right_idx"] >= 0].astype(np.int64)


def _median_place(sads):
    """(n, median, its first-level bin, its rank inside that bin, the bin's population)."""
    s = np.sort(sads)
    med = int(s[len(s) // 2])
    b = med >> 8
    return len(s), med, b, len(s) // 2 - int((s >> 8 < b).sum()), int((s >> 8 == b).sum())


def test_windows_reach_every_instance_under_one_pass_and_more():
    seen = set()
    for g in PC.edge_groups():
        if g["name"].startswith("windows"):
            cfg = R._config(g["cfg"])
            w, L = cfg["sad_half_window"], cfg["sad_slide"]
            for p, c in enumerate(g["pairs"]):
                matched = int((PC.edge_restatement(g["name"], p)[0]["right_idx"] >= 0).sum())
                refused = len(c["expect"]) - matched
                assert matched >= 8 and refused >= 2 and len(_trace(g, c)) == matched, (g["name"], matched, refused)
                seen.add((w, -(-(2 * L + 1) // 16)))
    assert {w for w, _ in seen} == set(range(1, 8))
    assert all((w, 1) in seen and (w, 2) in seen for w in range(1, 8)) and (7, 3) in seen
    # the row forms of load_row<w>: 2w + 1 bytes as full dwords and a tail shifted down by 8 (4 - rem) bits, or three single bytes
    assert {w: ((2 * w + 1) >> 2, (2 * w + 1) & 3) for w in range(1, 8)} == {1: (0, 3), 2: (1, 1), 3: (1, 3), 4: (2, 1), 5: (2, 3), 6: (3, 1), 7: (3, 3)}


def test_slides_reach_every_index_pass_and_tie():
    lanes_of_last_pass = {}
    for L in PC.SLIDE_TIES:
        g = GROUPS["slide L=%d" % L]
        idx, ties = g["pairs"]
        tr = _trace(g, idx)
        obs = PC.edge_restatement(g["name"], 0)[0]
        assert sorted(k for _, _, _, k in tr) == list(range(2 * L + 1))           # every index is a best index once
        for i, _, sad, k in tr:
            assert (sad == 0).sum() == 1 and (obs["right_idx"][i] >= 0) == (1 <= k <= 2 * L - 1)
        lanes_of_last_pass[L] = (2 * L + 1) - 16 * ((2 * L) // 16)
        tt = _trace(g, ties)
        assert len(tt) == len(PC.SLIDE_TIES[L])
        tobs = PC.edge_restatement(g["name"], 1)[0]
        for (per, k0), (i, _, sad, k) in zip(PC.SLIDE_TIES[L], tt):
            zeros = np.flatnonzero(sad == 0).tolist()
            assert zeros == list(range(k0, 2 * L + 1, per)) and len(zeros) >= 2 and k == k0, (L, per, k0, zeros)
            assert (tobs["right_idx"][i] >= 0) == (k0 >= 1) and (k0 == 0 or tobs["sad"][i] == 0)
    assert lanes_of_last_pass == {1: 3, 7: 15, 8: 1, 15: 15, 16: 1}               # 3, 15, 17, 31 and 33 shifts
    passes = lambda L: [{z >> 4 for z in range(k0, 2 * L + 1, per)} for per, k0 in PC.SLIDE_TIES[L]]   # noqa: E731
    assert {0, 1} in passes(16) and {0, 1, 2} in passes(16) and {0} in passes(7) and {0, 1} in passes(8) and {0, 1} in passes(15)
    assert (4, 3) in PC.SLIDE_TIES[16]                                             # 3, 7, 11, 15: four zeros inside pass 0, more beyond
    # the neighbours of the best index across the passes at L = 16: d1 of 16 and d3 of 15 and 31 come from another pass
    m16 = {k for i, _, _, k in _trace(GROUPS["slide L=16"], GROUPS["slide L=16"]["pairs"][0]) if 1 <= k <= 31}
    assert {14, 15, 16, 17, 30, 31} <= m16


def test_den_is_never_zero():
    """den == 0 of step 3 cannot occur (module docstring of stereo_cases): asserted on every slide of every group."""
    n = 0
    for g in PC.edge_groups():
        for c in g["pairs"]:
            for _, _, sad, k in _trace(g, c):
                if 0 < k < len(sad) - 1:
                    assert 2 * (int(sad[k - 1]) + int(sad[k + 1]) - 2 * int(sad[k])) >= 2
                    n += 1
    assert n > 3000


def _row_key(y, h):
    return np.fmin(np.fmax(np.floor(np.asarray(y, np.float32)), _F(0)), _F(h - 1)).astype(np.int64)


def _span_of(g, c, i):
    """(lo, hi) of the kernel's candidate span of left keypoint i: the rows within the widest band of the allowed octaves, +-1."""
    cfg = R._config(g["cfg"])
    h = g["height"]
    omax = min(max(int(c["kp_l"]["octave"][i]) + cfg["max_octave_diff"], 0), 7)
    rmax = _F(cfg["band_factor"]) * R.level_scales()[omax]
    y = c["kp_l"]["y"][i]
    lo = int(min(max(np.floor(y - rmax) - _F(1), _F(0)), _F(h - 1)))
    hi = int(min(max(np.floor(y + rmax) + _F(1), _F(0)), _F(h - 1)))
    return lo, hi


def test_rows_reach_every_chunk_shape():
    chunks = {}
    for h in PC.ROW_HEIGHTS:
        g = GROUPS["rows H=%d" % h]
        c = g["pairs"][0]
        chunk = -(-h // 256)
        chunks[h] = chunk
        rows = set(_row_key(c["kp_r"]["y"], h).tolist())
        assert set(PC.chunk_rows(h)) <= rows and {0, h - 1} <= rows
        for y in g["reach"]["probes"]:
            i = next(i for i in range(len(c["kp_l"])) if c["kp_l"]["y"][i] == y and c["expect"][i] and c["expect"][i][1] == 8
                     and c["kp_r"]["y"][c["expect"][i][0]] != y)
            lo, hi = _span_of(g, c, i)
            assert (lo, hi) == (max(y - 4, 0), min(y + 3, h - 1))
            copies = np.flatnonzero((c["desc_r"] == c["desc_l"][i]).all(1))
            assert set(_row_key(c["kp_r"]["y"][copies], h).tolist()) == {r for r in (lo - 1, lo, y - 3, hi, hi + 1) if 0 <= r < h and abs(r - y) > 2}
    assert chunks == {3: 1, 255: 1, 256: 1, 257: 2, 480: 2, 4096: 16}
    assert 257 % 2 == 1 and 128 * 2 < 257 < 129 * 2          # H = 257: thread 128's chunk is clipped, threads 129.. start beyond H
    assert 240 * 2 == 480 and 3 == 1 + 2 * 1                  # H = 480: threads 240.. are empty; H = 3 is the smallest legal image (w = 1)
    assert len(GROUPS["rows H=4096"]["pairs"][0]["kp_r"]) >= 512


def test_span_reaches_the_steps_lanes_and_the_lds_limit():
    g = GROUPS["span 8192"]
    c = g["pairs"][0]
    rows = _row_key(c["kp_r"]["y"], g["height"])
    assert len(rows) == g["kp_stride"] == 8192 and rows.tolist() == [PC.span_row(j) for j in range(8192)]
    end = np.cumsum(np.bincount(rows, minlength=g["height"]))                       # row ends of the counting sort
    start = end - np.bincount(rows, minlength=g["height"])
    obs = PC.edge_restatement(g["name"], 0)[0]
    spans, first_slot, last_step, later_step = set(), 0, 0, 0
    best, dist = R.best_candidates(c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **g["cfg"])
    for i in range(len(c["kp_l"])):
        lo, hi = _span_of(g, c, i)
        s, e = (int(end[lo - 1]) if lo else 0), int(end[hi])
        spans.add(e - s)
        j = int(obs["right_idx"][i])
        assert j == best[i] >= 0
        steps = -(-(e - s) // 64)
        if start[rows[j]] == s and end[rows[j]] == s + 1:
            first_slot += 1                                                          # slot s: lane 0, candidate 0 of step 0
        if (e - s) % 64 and start[rows[j]] - s >= 64 * (steps - 1):
            last_step += 1                                                           # wherever it lies in its row: the partial step
        same = [int(k) for k in np.flatnonzero((c["desc_r"] == c["desc_r"][j]).all(1))]
        if len(same) > 1:
            assert j == min(same) and dist[i] == 4
            later_step += any((start[rows[j]] - s) // 64 > (end[rows[k]] - 1 - s) // 64 for k in same)
    assert spans == {8192, 8191} and first_slot == 1 and last_step == 2 and later_step >= 1
    assert 8191 in obs["right_idx"] and len(c["kp_l"]) >= 560
    assert -(-8192 // 64) == 128 and 8191 % 64 == 63
    assert PC.match_lds_bytes(g) == 147456 > PC.LDS_DEFAULT
    twin = GROUPS["span twin kp_stride=1"]
    assert twin["kp_stride"] == 1 and twin["height"] == 4096 and PC.match_lds_bytes(twin) == 16400
    assert PC.match_lds_bytes(GROUPS["counts nL=8192"]) == 131328 > PC.LDS_DEFAULT
    # the older tests stay below both: 500 features at 320 x 240
    assert 4 * 240 + 16 * 8192 > PC.LDS_DEFAULT > 4 * 240 + 16 * 1024


def test_median_reaches_its_bins_and_ranks():
    place = {c["name"]: _median_place(_prefilter_sads(g, c)) for g in PC.edge_groups() if g["name"].startswith("median") for c in g["pairs"]}
    for k, v in place.items():
        print("%-48s n %d  median %5d  bin %3d  rank in bin %d of %d" % ((k,) + v))
    assert place["median n=1, bin 0, rank 0"] == (1, 3, 0, 0, 1)
    assert place["median n=2"][:2] == (2, 9) and place["median n=3"][:2] == (3, 9)
    assert place["median bin 156, first of its bin"] == (5, 40000, 156, 0, 3)
    assert place["median last of its bin"] == (5, 259, 1, 2, 3)
    assert place["median all equal"] == (4, 77, 0, 2, 4)
    assert place["median the largest SAD alone"] == (1, 57374, 224, 0, 1)
    assert place["median the largest SAD as the median"] == (3, 57374, 224, 0, 2)
    assert place["median (float)sad == 2.1f * 10 = 21 in fp32"][:2] == (5, 10)
    assert _F(2.1) * _F(10) == _F(21) and float(_F(2.1)) * 10 < 21              # equal in fp32 only: in fp64 the 21 would go
    assert place["median 10 == 2.5 * 4"][:2] == (5, 4) and place["median factor 0 keeps zeros"][:2] == (5, 0)
    assert place["median factor 0 drops all"][:2] == (3, 2)
    assert 57374 == 15 * 15 * 255 - 1


def test_counts_reach_every_round_shape():
    g = GROUPS["counts"]
    assert [len(c["kp_l"]) for c in g["pairs"]] == [15, 16, 17, 255, 256, 257]
    big = GROUPS["counts nL=8192"]["pairs"][0]
    alive = np.array([e is not None for e in big["expect"]]).reshape(32, 256).sum(1)
    assert len(big["kp_l"]) == 8192 and len(big["kp_r"]) == 16
    assert all(alive[r] == 256 for r in PC.COUNTS_DENSE) and all(alive[r] == 0 for r in PC.COUNTS_ABSENT)
    assert set(alive.tolist()) - {0, 256} == {51, 52}


def test_ends_reach_the_limits_of_the_config():
    cfgs = [R._config(g["cfg"]) for g in PC.edge_groups() if g["name"].startswith("ends")]
    assert {c["max_octave_diff"] for c in cfgs} == {0, 1, 8} and {c["th_hamming"] for c in cfgs} == {0, 75, 256, 257}
    assert {c["band_factor"] for c in cfgs} == {0.0, 2.0, 4.0, 1.0e9}
    k = GROUPS["ends default"]["pairs"][0]
    octs = set(k["kp_l"]["octave"].tolist()) | set(k["kp_r"]["octave"].tolist())
    assert {PC.INT_MAX, PC.INT_MIN, -5, -3, 9, 11} <= octs and np.abs(k["kp_l"]["x"]).max() > 2.0e9
    c = GROUPS["ends band_factor=1e9"]
    assert _span_of(c, c["pairs"][0], 0) == (0, c["height"] - 1)


def test_scale_keys_reach_every_byte_sign_and_round():
    g = PC.scale_groups()[0]
    recs = {r["name"]: r for r in g["records"]}
    for k in range(8):
        r = recs["key byte %d" % k]
        assert PC.first_differing_byte(r["used"]) == k and r["expect"][2] == 1
        if k >= 2:                                                                  # nothing but byte k differs
            keys = [PC.order_key(v) for v in r["used"]]
            assert len({key & ~(255 << (56 - 8 * k)) for key in keys}) == 1 and len(set(keys)) == len(keys) == 11
    keys = [PC.order_key(v) for v in (-np.inf, -2.0, -5e-324, -0.0, 0.0, 5e-324, 2.0, np.inf)]
    assert keys == sorted(keys) and len(set(keys)) == 8
    assert [recs[n]["expect"] for n in ("median negative", "median zero", "median positive")] == [(1.0, 5, 0), (1.0, 5, 0), (1.0, 5, 1)]
    assert recs["signed zeros"]["expect"] == (1.0, 5, 0) and recs["signed zeros below a positive median"]["expect"] == (2.0, 5, 1)
    assert np.signbit(recs["signed zeros"]["s"]).sum() == 2
    assert recs["ties around the rank"]["expect"] == (2.0, 7, 1) and recs["ties: the rank is the first of the upper run"]["expect"] == (2.0, 6, 1)
    assert recs["even n"]["expect"] == (4.0, 6, 1) and recs["odd n"]["expect"] == (4.0, 7, 1)
    assert recs["n_used = min_scale_matches - 1"]["expect"] == (1.0, 4, 0) and recs["n_used = min_scale_matches"]["expect"][1:] == (5, 1)
    assert recs["invalid pose record"]["expect"] == (1.0, 0, 0) and recs["no match"]["expect"] == (1.0, 0, 0)
    r = recs["mask removes whole rounds"]
    live = (r["mask"] != 0).reshape(-1)
    rounds = [int(live[a:a + 256].sum()) for a in range(0, 1000, 256)]
    assert rounds[1] == rounds[3] == 0 and rounds[0] > 200 and rounds[2] > 200 and r["expect"][1] == len(r["used"]) < sum(rounds)
    assert [x["query_is_first"] for x in PC.scale_groups()] == [True, False, True]
    full = PC.scale_groups()[2]
    assert full["match_cap"] == 8192 and 8 * full["match_cap"] == PC.LDS_DEFAULT and len(full["records"][0]["s"]) == 8192
    assert full["records"][0]["expect"] == ((4096 - 3000.0) * 0.25, 8192, 1) and full["records"][1]["expect"] == (1.0, 8191, 0)


def test_every_group_is_of_a_size_the_gpu_test_can_afford():
    """One workgroup per pair: the candidate tests nL x nR, the slides and the image bytes of a group bound its time."""
    for g in PC.edge_groups():
        tests = sum(len(c["kp_l"]) * len(c["kp_r"]) for c in g["pairs"])
        slides = sum(len(c["kp_l"]) for c in g["pairs"])
        assert tests <= 600 * 8192 and slides <= 8192 and len(g["pairs"]) <= 9, g["name"]
        assert 2 * len(g["pairs"]) * g["width"] * g["height"] <= 1 << 20, g["name"]
        assert 1 <= g["kp_stride"] <= 8192 and g["width"] <= 128 and g["height"] <= 4096
    assert len(PC.edge_groups()) == 43 and sum(len(g["pairs"]) for g in PC.edge_groups()) <= 80
