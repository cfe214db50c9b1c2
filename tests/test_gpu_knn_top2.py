"""Planted neighbours at every pair of accumulator positions of the matrix-core kNN-2 kernels (knn2_mfma.hip).

The running top-2 of a lane sees the 16 keys of an accumulator in groups of four (top2_quad). Which two of a query's keys are
the best and the runner-up decides which operand slots of that update carry them, so the planted sets below put the two in
every pair of positions: the same pair, the same quad, different quads, the other lane half, the other row tile, the other
train tile -- in both orders -- with every other train at one common, larger distance (a 62- or 126-fold tie).

Block trains: train r of N has the 256 / N bits of block r set.
  N = 64   query (i, j): 4 bits in block i, 3 in block j, 1 in every other block  ->  distances 65 to i, 67 to j, 71 to the rest;
           all 64 * 63 ordered pairs
  N = 128  query (i, j): 2 bits in block i, 1 in block j                          ->  distances 1, 3 and 5;
           j = (i + k) mod 128 for k in K128
  N = 64 + 32 all-ones trains (nt = 96: a padded second tile; 187 to the all-ones trains)
plus the first 1 and 2 trains of the N = 64 set (no runner-up / exactly one) and the N = 64 trains spread over 4100 rows of
all-ones trains (the 16-bit-index key layout of train sets beyond 4096).

Every comparison is exact: the expected answers are closed forms, and the oracle must agree with them.

The library under test is the one the binding loads, so the same file also runs against other builds:
test_other_builds_pass_the_same_checks starts it once on the per-distance build (-DARIA_KNN_TOP2_SINGLE=1) and once on the
variants library with ARIA_KNN_IMPL=int8."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K128 = (1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127)
WIDE_ROWS = 4100


def _pack(bits):
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")


def _block_trains(n):
    w = 256 // n
    bits = np.zeros((n, 256), np.uint8)
    for r in range(n):
        bits[r, w * r:w * (r + 1)] = 1
    return bits


def _planted(n, pairs, hits_i, hits_j, hits_rest):
    w = 256 // n
    bits = np.zeros((len(pairs), 256), np.uint8)
    if hits_rest:
        bits[:, ::w] = 1                                   # the first bit of every block
    for row, (i, j) in enumerate(pairs):
        bits[row, w * i:w * (i + 1)] = 0
        bits[row, w * j:w * (j + 1)] = 0
        bits[row, w * i:w * i + hits_i] = 1
        bits[row, w * j:w * j + hits_j] = 1
    return bits


class Planted:
    """name, queries q, trains t, the planted (best, runner-up) train rows and distances, and two ratios that bracket
    best / runner-up: `lo` must match nothing, `hi` every query."""

    def __init__(self, name, q, t, idx, d1, d2, lo, hi):
        self.name, self.q, self.t = name, _pack(q), _pack(t)
        self.idx = np.asarray(idx, np.int32)
        self.dist = np.tile(np.array([d1, d2], np.int32), (len(idx), 1))
        self.lo, self.hi = lo, hi
        assert float(np.float32(d1)) >= float(np.float32(lo) * np.float32(d2)) and np.float32(d1) < np.float32(hi) * np.float32(d2)


@pytest.fixture(scope="module")
def sets():
    p64 = [(i, j) for i in range(64) for j in range(64) if i != j]
    p128 = [(i, (i + k) % 128) for i in range(128) for k in K128]
    t64, q64 = _block_trains(64), _planted(64, p64, 4, 3, 1)
    t96 = np.concatenate([t64, np.ones((32, 256), np.uint8)])
    rows = 65 * np.arange(64) + 3                          # the block trains among 4100 all-ones rows, every 65th row
    twide = np.ones((WIDE_ROWS, 256), np.uint8)
    twide[rows] = t64
    out = {
        "n64": Planted("n64", q64, t64, p64, 65, 67, 0.96, 0.98),
        "n128": Planted("n128", _planted(128, p128, 2, 1, 0), _block_trains(128), p128, 1, 3, 0.3, 0.5),
        "n96": Planted("n96", q64, t96, p64, 65, 67, 0.96, 0.98),
        "wide": Planted("wide", q64, twide, rows[np.asarray(p64)], 65, 67, 0.96, 0.98),
    }
    for s in out.values():
        s.q.setflags(write=False)
        s.t.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _want_matches(aria, s, ratio):
    """Closed form of the ratio test on a planted set: every query matches its best train at `hi`, none at `lo`."""
    if ratio == s.lo:
        return np.zeros(0, aria.MATCH_DTYPE)
    out = np.zeros(len(s.q), aria.MATCH_DTYPE)
    out["query_idx"], out["train_idx"], out["distance"] = np.arange(len(s.q)), s.idx[:, 0], s.dist[:, 0]
    return out


@pytest.mark.parametrize("name", ["n64", "n128", "n96", "wide"])
def test_host_entry_finds_the_planted_pair(aria, oracle, sets, name):
    """aria_matcher_knn2 (256-query workgroups) and aria_matcher_match (the same kernel over slices of train tiles, merged
    by the ratio kernel) against the closed form and the oracle."""
    s = sets[name]
    m = aria.HipMatcher(max_query=4096, max_train=max(4096, len(s.t)))
    try:
        idx, dist = m.knn2(s.q, s.t)
        oidx, odist = oracle.knn2(s.q, s.t)
        assert np.array_equal(oidx, s.idx) and np.array_equal(odist, s.dist), "the oracle disagrees with the closed form"
        bad = np.flatnonzero((idx != s.idx).any(1) | (dist != s.dist).any(1))
        assert len(bad) == 0, "%d queries, first %d: got %s %s want %s %s" % (len(bad), bad[0], idx[bad[0]], dist[bad[0]],
                                                                             s.idx[bad[0]], s.dist[bad[0]])
        for ratio in (s.lo, s.hi):
            got = m.match(s.q, s.t, None, ratio)
            assert got.tobytes() == _want_matches(aria, s, ratio).tobytes(), "ratio %g" % ratio
            assert got.tobytes() == oracle.match_ratio(s.q, s.t, ratio).tobytes(), "ratio %g (oracle)" % ratio
    finally:
        m.close()


@pytest.mark.parametrize("nt", [1, 2])
def test_host_entry_with_one_and_two_trains(aria, oracle, sets, nt):
    """nt = 1: no runner-up (index -1) and no match at any ratio; nt = 2: the runner-up is the other train."""
    s = sets["n64"]
    t = s.t[:nt]
    m = aria.HipMatcher()
    try:
        idx, dist = m.knn2(s.q, t)
        oidx, odist = oracle.knn2(s.q, t)
        assert np.array_equal(idx, oidx) and np.array_equal(dist, odist)
        hit = np.flatnonzero(s.idx[:, 0] == 0)             # queries whose planted best is train 0
        assert (idx[hit, 0] == 0).all() and (dist[hit, 0] == 65).all()
        if nt == 1:
            assert (idx[:, 0] == 0).all() and (idx[:, 1] == -1).all()
        else:
            assert (np.sort(idx, axis=1) == [0, 1]).all() and (dist[:, 0] <= dist[:, 1]).all()
        for ratio in (0.75, 0.98, 1.0):
            assert m.match(s.q, t, None, ratio).tobytes() == oracle.match_ratio(s.q, t, ratio).tobytes()
    finally:
        m.close()


def _chunks(nq, size):
    return [(a, min(a + size, nq)) for a in range(0, nq, size)]


@pytest.mark.parametrize("name", ["n64", "n128", "n96"])
def test_batch_entry_finds_the_planted_pair(aria, oracle, torch_cuda, sets, name):
    """aria_matcher_match_batch_device over 1024 pairs of at most 512 queries -- enough workgroups for the 512-query kernel.
    Pair p takes the p-th 512-query chunk of the set (cyclically) against the whole train set, except pairs 5 and 6, which
    see only the first 1 and 2 trains. At `lo` nothing may match, at `hi` every query must."""
    torch = torch_cuda
    s, dev, cap, n_pairs = sets[name], torch.device("cuda", 0), 512, 1024
    ch = _chunks(len(s.q), cap)
    Q = np.zeros((len(ch), cap, 32), np.uint8)
    for c, (a, b) in enumerate(ch):
        Q[c, :b - a] = s.q[a:b]
    T = np.zeros((cap, 32), np.uint8)
    T[:len(s.t)] = s.t
    which = np.arange(n_pairs) % len(ch)
    nq = np.array([ch[c][1] - ch[c][0] for c in which], np.int32)
    nt = np.full(n_pairs, len(s.t), np.int32)
    nt[5], nt[6] = 1, 2
    dQ = torch.from_numpy(Q).to(dev)[torch.from_numpy(which).to(dev)].contiguous()
    dT = torch.from_numpy(T).to(dev).unsqueeze(0).repeat(n_pairs, 1, 1).contiguous()
    dnq, dnt = torch.from_numpy(nq).to(dev), torch.from_numpy(nt).to(dev)
    m = aria.HipMatcher()
    try:
        for ratio in (s.lo, s.hi):
            dM = torch.zeros((n_pairs, cap, 3), dtype=torch.int32, device=dev)
            dN = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()                       # the matcher runs on a stream of its own
            m.match_batch_device(dQ, dnq, dT, dnt, n_pairs, cap * 32, ratio, dM, dN, cap)
            m.sync()
            M = dM.cpu().numpy().view(aria.MATCH_DTYPE).reshape(n_pairs, cap)
            N = dN.cpu().numpy()
            full = {}
            for c, (a, b) in enumerate(ch):
                full[c] = oracle.match_ratio(s.q[a:b], s.t, ratio)
                want = _want_matches(aria, s, ratio)
                if len(want):
                    want = want[a:b].copy()
                    want["query_idx"] -= a
                assert full[c].tobytes() == want.tobytes(), "the oracle disagrees with the closed form"
            for p in range(n_pairs):
                a, b = ch[which[p]]
                want = full[which[p]] if p not in (5, 6) else oracle.match_ratio(s.q[a:b], s.t[:nt[p]], ratio)
                assert N[p] == len(want) and M[p, :N[p]].tobytes() == want.tobytes(), "pair %d at ratio %g" % (p, ratio)
    finally:
        m.close()


def test_batch_entry_wide_layout(aria, oracle, torch_cuda, sets):
    """Two pairs in 4100-row slots: the kernel of the 16-bit-index key layout (one shift-add per key before the update)."""
    torch = torch_cuda
    s, dev, rows = sets["wide"], torch.device("cuda", 0), WIDE_ROWS
    Q = np.zeros((2, rows, 32), np.uint8)
    Q[0, :len(s.q)] = s.q
    Q[1, :1000] = s.q[-1000:]
    nq, nt = np.array([len(s.q), 1000], np.int32), np.array([rows, rows], np.int32)
    dQ = torch.from_numpy(Q).to(dev)
    dT = torch.from_numpy(np.stack([s.t, s.t])).to(dev)
    m = aria.HipMatcher(max_query=rows, max_train=rows)
    try:
        for ratio in (s.lo, s.hi):
            dM = torch.zeros((2, rows, 3), dtype=torch.int32, device=dev)
            dN = torch.zeros(2, dtype=torch.int32, device=dev)
            dnq, dnt = torch.from_numpy(nq).to(dev), torch.from_numpy(nt).to(dev)
            torch.cuda.synchronize()
            m.match_batch_device(dQ, dnq, dT, dnt, 2, rows * 32, ratio, dM, dN, rows)
            m.sync()
            M, N = dM.cpu().numpy().view(aria.MATCH_DTYPE).reshape(2, rows), dN.cpu().numpy()
            for p in range(2):
                want = oracle.match_ratio(Q[p, :nq[p]], s.t, ratio)
                assert len(want) == (nq[p] if ratio == s.hi else 0)
                assert N[p] == len(want) and M[p, :N[p]].tobytes() == want.tobytes(), "pair %d at ratio %g" % (p, ratio)
    finally:
        m.close()


@pytest.mark.parametrize("name,n_kf", [("n64", 128), ("n128", 352), ("n96", 128), ("n64", 3), ("wide", 2)])
def test_db_scan_counts_the_planted_pairs(aria, oracle, torch_cuda, sets, name, n_kf):
    """aria_matcher_match_db_device (the kernels' counting mode, double-precision ratio): one query set against n_kf copies
    of the train set -- 512-query workgroups where n_kf is large, 256-query ones at n_kf = 3 --, keyframes 1 and 2 cut to
    one and two trains. Good matches: none at `lo`, every query at `hi`; at the loop detector's 0.7 whatever the oracle counts."""
    torch = torch_cuda
    s, dev = sets[name], torch.device("cuda", 0)
    rows = len(s.t) if name == "wide" else 128
    T = np.zeros((rows, 32), np.uint8)
    T[:len(s.t)] = s.t
    cnt = np.full(n_kf, len(s.t), np.int32)
    cnt[1] = 1
    if n_kf > 2:
        cnt[2] = 2
    dQ = torch.from_numpy(s.q.copy()).to(dev)
    dT = torch.from_numpy(T).to(dev).unsqueeze(0).repeat(n_kf, 1, 1).contiguous()
    dC = torch.from_numpy(cnt).to(dev)
    m = aria.HipMatcher(max_query=4096, max_train=max(4096, rows))
    try:
        for ratio in (s.lo, s.hi, 0.7):
            dG = torch.full((n_kf,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            m.match_db_device(dQ, len(s.q), dT, dC, n_kf, rows * 32, ratio, dG)
            m.sync()
            G = dG.cpu().numpy()
            by_count = {int(c): oracle.count_good_matches_f64(s.q, s.t[:c], ratio) for c in set(cnt.tolist())}
            if ratio in (s.lo, s.hi):
                assert by_count[len(s.t)] == (len(s.q) if ratio == s.hi else 0), "the oracle disagrees with the closed form"
            assert by_count[1] == 0
            assert np.array_equal(G, np.array([by_count[int(c)] for c in cnt], np.int32)), "ratio %g" % ratio
    finally:
        m.close()


# ---- the same checks on the other builds of the update --------------------------------------------------------------------------
def _single_build():
    """Product flags plus -DARIA_KNN_TOP2_SINGLE=1 (tools/build_ab.sh), rebuilt when a source is newer."""
    lib = os.path.join(ROOT, "build", "ab", "libknn_top2_single.so")
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp", ".inc")))
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        subprocess.check_call([os.path.join(ROOT, "tools", "build_ab.sh"), "knn_top2_single", "-DARIA_KNN_TOP2_SINGLE=1"],
                              stdout=subprocess.DEVNULL)
    return lib, {}


def _int8_variant():
    sys.path.insert(0, ROOT)
    import aria_slam_amd
    return aria_slam_amd.build_variants_library(), {"ARIA_KNN_IMPL": "int8"}


@pytest.mark.parametrize("build", [_single_build, _int8_variant], ids=["per_distance_build", "variants_int8"])
def test_other_builds_pass_the_same_checks(build):
    lib, env = build()
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = lib
    e.update(env)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                          "-k", "not other_builds"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout and "skipped" not in out.stdout, out.stdout[-2000:]
