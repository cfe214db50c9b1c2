"""Guided matching at every limit and size the C-ABI admits (tests/proj_cases.py, edge_groups()), without a GPU: the restatement
aria_slam_amd/proj_ref.py against the answers written down from the construction, against its literal triple loop, a census
asserting that the groups reach what they claim to reach, and wrong copies of the definition showing that the new cases see
mistakes the case table cannot.

The triple loop runs where keypoints x live landmarks <= TRIPLE_CUT (everything but index_bits and the 8192-keypoint span); a
dead landmark is never visible, so a range is looped over as its live landmarks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_cases as PC   # noqa: E402
from aria_slam_amd import proj_ref as R   # noqa: E402

TRIPLE_CUT = 5000
_F = np.float32


def _frames():
    return [pytest.param(g, f, id="%s / %s" % (g["name"], f["name"])) for g in PC.edge_groups() for f in g["frames"]]


def _live(g, f):
    """(landmarks of the frame's range that are alive, their i)."""
    lm = g["landmarks"][f["first"]:f["first"] + f["count"]]
    i = np.flatnonzero(lm["octave"] >= 0)
    return lm[i], i


@pytest.mark.parametrize("g,f", _frames())
def test_restatement_equals_the_written_answers(g, f):
    assert g["written"]                                                       # every group of today has them
    obs, corr, pairs = PC.edge_restatement(g, f)
    want_obs, want_corr, want_pairs = PC.edge_expected(g, f)
    for name in obs.dtype.names:
        bad = np.flatnonzero(obs[name].view(np.int32) != want_obs[name].view(np.int32))
        assert len(bad) == 0, (g["name"], f["name"], name, bad[:8], obs[name][bad[:8]], want_obs[name][bad[:8]])
    assert corr.tobytes() == want_corr.tobytes() and pairs.tobytes() == want_pairs.tobytes()
    assert np.isfinite(obs["u"]).all() and np.isfinite(obs["v"]).all() and np.isfinite(corr["u"]).all() and np.isfinite(corr["v"]).all()


def test_claim_bits_compaction_is_the_full_range_on_a_prefix():
    """The restatement of claim_bits runs on the live landmarks alone. On the first 70000 records of the range, which hold
    seven of them and both sides of 2^16, the full loop gives the same records."""
    g = PC.edge_group("claim_bits")
    f = g["frames"][0]
    n = 70000
    kp, desc = PC.edge_frame_arrays(g, f)
    full = R.search_frame_ref(f["pose"], kp, desc, f["n"], g["kp_stride"], g["landmarks"], 0, n, n, g["cfg"], g["width"], g["height"])[0]
    lm = g["landmarks"][:n]
    live = np.flatnonzero(lm["octave"] >= 0)
    assert len(live) == 7
    o = R.search_ref(f["pose"], kp[:f["n"]], desc[:f["n"]], lm[live], g["cfg"], g["width"], g["height"])[0]
    want = R.not_visible_obs(n)
    want[live] = o
    assert full.tobytes() == want.tobytes()


@pytest.mark.parametrize("g,f", _frames())
def test_restatement_equals_a_literal_triple_loop(g, f):
    lm, i = _live(g, f)
    if len(f["kp"]) * len(lm) > TRIPLE_CUT:
        assert g["name"] in ("index_bits", "spans one cell")                  # the cut, stated: nothing else is left out
        return
    obs = PC.edge_restatement(g, f)[0]
    loop = R.search_triple_loop(f["pose"], f["kp"], f["desc"], lm, g["cfg"], g["width"], g["height"])
    assert obs[i].tobytes() == loop.tobytes()


# ---- census: what the groups reach, computed from the definition alone -----------------------------------------------------------
def _cell(x, n):
    """proj_cell of csrc/proj_search.hip in NumPy: monotone, total, a NaN in cell 0."""
    c = np.floor(np.asarray(x, np.float32) * _F(1.0 / 32.0))
    return np.fmin(np.fmax(c, _F(0)), _F(n - 1)).astype(np.int64)


def _census(g, f):
    """Per frame: the greatest k that is a best, a second, a claimed keypoint; the greatest i that wins and that loses a claim;
    the cells of the grid; the longest span of sorted entries one landmark walks in one cell row; whether a window covers a
    grid of more than one cell entirely; the flags values."""
    c = dict(R.DEFAULTS, **g["cfg"])
    gx, gy = (g["width"] + 31) >> 5, (g["height"] + 31) >> 5
    kp, desc = f["kp"][:f["n"]], f["desc"][:f["n"]]
    per_cell = np.bincount(_cell(kp["y"], gy) * gx + _cell(kp["x"], gx), minlength=gx * gy).reshape(gy, gx)
    obs = PC.edge_restatement(g, f)[0]
    out = dict(best=-1, second=-1, claimed=-1, wins=-1, loses=-1, cells=gx * gy, span=0, whole=False, flags=set(obs["flags"][:f["count"]].tolist()))
    lm, idx = _live(g, f)
    scale = R.level_scales()
    ok = np.clip(kp["octave"].astype(np.int64), 0, 7)
    for j, i in enumerate(idx):
        u, v, vis = R.project(f["pose"], lm["X"][j], lm["octave"][j], c, g["width"], g["height"])
        if not vis:
            continue
        oi = min(int(lm["octave"][j]), 7)
        r = _F(c["radius_px"]) * scale[oi]
        cx0, cx1, cy0, cy1 = _cell(u - r - _F(1), gx), _cell(u + r + _F(1), gx), _cell(v - r - _F(1), gy), _cell(v + r + _F(1), gy)
        out["span"] = max(out["span"], max(int(per_cell[cy, cx0:cx1 + 1].sum()) for cy in range(cy0, cy1 + 1)))
        out["whole"] |= gx * gy > 1 and (cx0, cx1, cy0, cy1) == (0, gx - 1, 0, gy - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            cand = np.flatnonzero((np.abs(ok - oi) <= c["max_octave_diff"]) & (np.abs(kp["x"] - u) <= r) & (np.abs(kp["y"] - v) <= r))
        if len(cand) == 0:
            continue
        order = sorted((int(R._POP[desc[k] ^ lm["desc"][j]].sum()), int(k)) for k in cand)
        out["best"] = max(out["best"], order[0][1])
        if len(order) > 1:
            out["second"] = max(out["second"], order[1][1])
        fl = int(obs["flags"][i])
        if fl & R.ACCEPTED:
            out["claimed"] = max(out["claimed"], order[0][1])
            key = "wins" if fl & R.WON else "loses"
            out[key] = max(out[key], int(i))
    return out


def test_census_the_groups_reach_what_they_claim():
    rows = {(g["name"], f["name"]): _census(g, f) for g in PC.edge_groups() for f in g["frames"]}
    for (gn, fn), c in rows.items():
        print("%-28s cells %5d  span %4d  whole %d  best k %4d  second k %4d  claimed k %4d  wins i %7d  loses i %7d  flags %s"
              % (gn, c["cells"], c["span"], c["whole"], c["best"], c["second"], c["claimed"], c["wins"], c["loses"], sorted(c["flags"])))
    top = lambda key: max(c[key] for c in rows.values())   # noqa: E731
    assert top("best") == top("second") == top("claimed") == R.MAX_KP - 1 == 8191
    assert top("wins") == R.MAX_LAND - 1 and top("loses") == (1 << 19) + 7 and min(top("wins"), top("loses")) >= 1 << 16
    assert {1, 2, 128, 16384, 80} <= {c["cells"] for c in rows.values()}
    assert top("span") >= 8192
    assert {80, 16384} <= {c["cells"] for c in rows.values() if c["whole"]}                  # a window that covers the whole grid
    old = PC.table()
    assert max(len(f["kp"]) for f in old["frames"]) == 301 and old["land_cap"] == 260          # what the case table reaches
    # every flags value under every configuration of `limits` where it can occur. th_hamming = 0 accepts nothing, so 7 and 15
    # cannot occur under it; every other value occurs under every configuration.
    for which in PC.LIMIT_CONFIGS:
        flags = rows[("limits " + which, "limits " + which)]["flags"]
        assert flags == ({0, 1, 3} if which == "th_hamming=0" else {0, 1, 3, 7, 15}), (which, flags)


def test_written_live_list_of_claim_bits():
    g = PC.edge_group("claim_bits")
    assert g["land_cap"] == g["frames"][0]["count"] == len(g["landmarks"]) == 1 << 20
    live = np.flatnonzero(g["landmarks"]["octave"] >= 0)
    assert tuple(live) == PC.CLAIM_LIVE and set((0, 3, 4095, 4096, 65535, 65536, 65541, 1 << 19, (1 << 20) - 1)) <= set(live.tolist())
    exp = g["frames"][0]["exp"]
    assert (exp["flags"][live] >= 7).all() and (np.delete(exp["flags"], live) == 0).all()
    g = PC.edge_group("index_bits")
    assert g["kp_stride"] == 8192 and all(f["n"] == 8192 for f in g["frames"])


# ---- wrong copies of the definition ------------------------------------------------------------------------------------------------
MISTAKES = {
    "index field of 12 bits in the key": "the top-2 key is distance << 12 | k",
    "index decoded with 12 bits": "kp_idx = m1 & 4095",
    "claim key shifted by 16": "the claim key is hamming << 16 | i",
    "i cut to 16 bits in the claim order": "hamming << 20 | (i & 0xFFFF) on both sides of the claim",
    "i cut to 19 bits in the claim order": "hamming << 20 | (i & 0x7FFFF) on both sides of the claim",
    "i cut to 19 bits by the claimant alone": "the atomic-min side cuts i, the resolving side does not",
    "window difference in fp64": "|xk - u| and |yk - v| taken in fp64",
    "image test before the cast": "0 <= u < width tested on the fp64 pixel",
    "octave difference fixed at 1": "max_octave_diff ignored",
    "hamming <= 255 assumed": "the distance kept in 8 bits",
    "radius not scaled by the level": "r = radius_px at every octave",
}

def _search_copy(pose, kp, desc, lm, idx, cfg, width, height, mistake=None):
    """A copy of proj_ref.project and proj_ref.search_ref in the integer-key form of the header's rules 3 and 5 (best and second
    are the two least of distance << 13 | k, a keypoint goes to the least hamming << 20 | i), with one mistake made on demand.
    idx: the i of each landmark. Returns obs alone. With mistake=None it is the definition (asserted below)."""
    assert mistake is None or mistake in MISTAKES
    c = dict(R.DEFAULTS, **cfg)
    scale = R.level_scales()
    fx, fy, cx, cy = (np.float64(v) for v in c["K"])
    P = np.asarray(pose, np.float64).reshape(12)
    xk, yk = kp["x"], kp["y"]
    okc = np.clip(kp["octave"].astype(np.int64), 0, 7)
    mod = 1 if mistake == "octave difference fixed at 1" else int(c["max_octave_diff"])
    kshift = 12 if mistake == "index field of 12 bits in the key" else 13
    kmask = 4095 if mistake in ("index field of 12 bits in the key", "index decoded with 12 bits") else 8191
    cshift = 16 if mistake == "claim key shifted by 16" else 20
    cut = {"i cut to 16 bits in the claim order": 0xFFFF, "i cut to 19 bits in the claim order": 0x7FFFF}.get(mistake, 0xFFFFF)
    cut_claimant = 0x7FFFF if mistake == "i cut to 19 bits by the claimant alone" else cut
    obs = R.not_visible_obs(len(lm))
    claims = {}
    for j in range(len(lm)):
        X = lm["X"][j].astype(np.float64)
        with np.errstate(all="ignore"):
            xc = [((P[4 * r] * X[0] + P[4 * r + 1] * X[1]) + P[4 * r + 2] * X[2]) + P[4 * r + 3] for r in range(3)]
            if not (int(lm["octave"][j]) >= 0) or not (xc[2] > np.float64(c["min_depth"])):
                continue
            u64, v64 = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
            u, v = _F(u64), _F(v64)
            if mistake == "image test before the cast":
                inside = u64 >= 0 and u64 < width and v64 >= 0 and v64 < height
            else:
                inside = u >= _F(0) and u < _F(width) and v >= _F(0) and v < _F(height)
            if not inside:
                continue
            o = obs[j]
            o["u"], o["v"], o["flags"] = u, v, R.VISIBLE
            oi = min(int(lm["octave"][j]), 7)
            r = _F(c["radius_px"]) if mistake == "radius not scaled by the level" else _F(c["radius_px"]) * scale[oi]
            if mistake == "window difference in fp64":
                near = (np.abs(xk.astype(np.float64) - np.float64(u)) <= np.float64(r)) & (np.abs(yk.astype(np.float64) - np.float64(v)) <= np.float64(r))
            else:
                near = (np.abs(xk - u) <= r) & (np.abs(yk - v) <= r)
        cand = np.flatnonzero((np.abs(okc - oi) <= mod) & near)
        if len(cand) == 0:
            continue
        dist = R._POP[desc[cand] ^ lm["desc"][j]].sum(axis=1).astype(np.int64)
        if mistake == "hamming <= 255 assumed":
            dist &= 255
        keys = np.sort((dist << kshift) | cand)
        m1, m2 = int(keys[0]), (int(keys[1]) if len(keys) > 1 else None)
        ham, second, kk = m1 >> kshift, (-1 if m2 is None else m2 >> kshift), m1 & kmask
        o["hamming"], o["second"], o["flags"] = ham, second, R.VISIBLE | R.CANDIDATES
        if ham >= int(c["th_hamming"]) or (second >= 0 and not (_F(ham) < _F(c["ratio"]) * _F(second))):
            continue
        o["flags"] |= R.ACCEPTED
        o["kp_idx"] = kk
        claims[kk] = min(claims.get(kk, 1 << 62), (ham << cshift) | (int(idx[j]) & cut_claimant))
    for j in range(len(lm)):
        o = obs[j]
        if o["flags"] & R.ACCEPTED:
            if claims[int(o["kp_idx"])] == (int(o["hamming"]) << cshift) | (int(idx[j]) & cut):
                o["flags"] |= R.WON
            else:
                o["kp_idx"] = -1
    return obs


def _copy_on_edges(mistake):
    out = []
    for g in PC.edge_groups():
        for f in g["frames"]:
            lm, i = _live(g, f)
            out.append(_search_copy(f["pose"], f["kp"][:f["n"]], f["desc"][:f["n"]], lm, i, g["cfg"], g["width"], g["height"], mistake).tobytes())
    return out


def _copy_on_table(mistake):
    t = PC.table()
    out = []
    for f in t["frames"]:
        if f["valid"]:
            lm = t["landmarks"][f["first"]:f["first"] + f["count"]]
            out.append(_search_copy(f["pose"], f["kp"][:f["n"]], f["desc"][:f["n"]], lm, np.arange(len(lm)), t["cfg"], t["width"], t["height"],
                                    mistake).tobytes())
    return out


@pytest.fixture(scope="module")
def faithful():
    """The copy without a mistake, on both tables; it must be the definition."""
    edges, table = _copy_on_edges(None), _copy_on_table(None)
    j = 0
    for g in PC.edge_groups():
        for f in g["frames"]:
            assert edges[j] == PC.edge_restatement(g, f)[0][_live(g, f)[1]].tobytes(), (g["name"], f["name"])
            j += 1
    t = PC.table()
    for b, f in zip(table, [f for f in t["frames"] if f["valid"]]):
        assert b == f["exp"].tobytes(), f["name"]
    return edges, table


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_a_wrong_copy_of_the_definition_differs_on_the_new_cases(faithful, mistake):
    edges, table = faithful
    got = _copy_on_edges(mistake)
    names = ["%s / %s" % (g["name"], f["name"]) for g in PC.edge_groups() for f in g["frames"]]
    seen_by = [n for n, a, b in zip(names, got, edges) if a != b]
    on_table = _copy_on_table(mistake) != table                               # recorded for DESIGN, never asserted in a direction
    print("%-42s (%s): case table %s; edge groups see it in: %s" % (mistake, MISTAKES[mistake], "SEES it" if on_table else "blind", "; ".join(seen_by)))
    assert seen_by, mistake
