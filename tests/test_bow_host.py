"""The definition of the place-recognition stage (aria_slam_amd/bow_ref.py) on the case table (tests/bow_cases.py), its bit
budget, its retrieval on a generated scene, and the host rules of KeyframeDB.find_candidates_bow. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_cases as BC   # noqa: E402
from aria_slam_amd import bow_ref as R   # noqa: E402
from aria_slam_amd.loopdb import score_candidates   # noqa: E402


@pytest.mark.parametrize("F,n_w,want", BC.ILOG)
def test_integer_logarithm_literals(F, n_w, want):
    assert R.ilog2_q8(F, n_w) == want


@pytest.mark.parametrize("F,n_w,want", BC.IDF)
def test_weight_literals(F, n_w, want):
    assert R.idf_weight(F, n_w) == want


def test_integer_logarithm_stays_below_4096_and_is_monotone():
    prev = 0
    for n_w in range(65535, 0, -257):
        v = R.ilog2_q8(65535, n_w)
        assert prev <= v < 4096
        prev = v


@pytest.mark.parametrize("c", BC.train_cases(), ids=lambda c: c["name"])
def test_train_cases(c):
    if c.get("refused"):
        with pytest.raises(ValueError):
            R.train(c["frames"], c["V"], c["iters"])
        return
    words, idf, run = R.train(c["frames"], c["V"], c["iters"])
    assert words.tobytes() == np.array(c["words"], np.uint8).tobytes()
    assert idf.tolist() == list(c["idf"]) and idf.dtype == np.uint16
    assert run == c["run"]


@pytest.mark.parametrize("c", BC.transform_cases(), ids=lambda c: c["name"])
def test_transform_cases(c):
    words, idf = np.array(c["words"], np.uint8), np.array(c["idf"], np.uint16)
    for f, (cnt, desc) in enumerate(zip(c["counts"], c["frames"])):
        valid = 0 <= cnt <= c["rows"]
        tf, N = R.transform(desc[:cnt] if valid else desc[:0], words, idf)
        assert tf.tolist() == c["tf"][f] and N == c["norm"][f], (c["name"], f)
    assert c["error"] == any(not 0 <= cnt <= c["rows"] for cnt in c["counts"])


@pytest.mark.parametrize("c", BC.query_cases(), ids=lambda c: c["name"])
def test_query_cases(c):
    ix = R.BowIndexRef(BC.QUERY_WORDS, BC.QUERY_IDF, c["capacity"], c["top_k"], c["mfb"])
    for kid, tf in c["entries"]:
        ix.add_bag(kid, tf, sum(tf))
    assert ix.size() == c["size"]
    for index, kid, norm in c["info"]:
        assert ix.info(index) == (kid, norm)
    for qid, tf, count, hits in c["queries"]:
        got, n = ix.query_bag(qid, np.array(tf, np.uint16), sum(tf))
        assert n == count and got.tobytes() == BC.expected_hits(hits).tobytes(), (c["name"], qid, tf, got)


def test_bit_budget_worst_case():
    """rows = 4096 descriptors on one word of weight 4095: the norm stays below 2^24, the numerator below 2^48, and the one
    division is exact to its rounding (here: exactly 1.0, and 1 / 3 for a third of it)."""
    idf = np.array([4095, 4095], np.uint16)
    tf = np.array([4096, 0], np.uint16)
    N = R.norm_of(tf, idf)
    assert N == 4096 * 4095 < 2 ** 24
    S, sc = R.score(tf, N, tf, N, idf)
    assert S == N * N < 2 ** 48 and sc == 1.0
    assert float(S) == S and float(N * N) == N * N                      # both operands of the division are exact doubles
    other = np.array([2048, 2048], np.uint16)                           # the same norm, half of its mass on the shared word
    No = R.norm_of(other, idf)
    S2, sc2 = R.score(tf, N, other, No, idf)
    assert No == N and 2 * S2 == N * N and sc2 == 0.5


def test_identical_and_disjoint_bags():
    idf = np.array([3, 1, 0, 9], np.uint16)
    a, b = np.array([2, 5, 7, 0], np.uint16), np.array([0, 0, 4, 6], np.uint16)
    Na, Nb = R.norm_of(a, idf), R.norm_of(b, idf)
    assert R.score(a, Na, a, Na, idf) == (Na * Na, 1.0)
    assert R.score(a, Na, b, Nb, idf) == (0, 0.0)                       # they share only the word of weight 0


def test_score_is_the_l1_score():
    rng = np.random.default_rng(1)
    idf = rng.integers(0, 4096, 64).astype(np.uint16)
    for _ in range(20):
        a, b = rng.integers(0, 9, 64).astype(np.uint16), rng.integers(0, 9, 64).astype(np.uint16)
        Na, Nb = R.norm_of(a, idf), R.norm_of(b, idf)
        va, vb = a.astype(np.float64) * idf / Na, b.astype(np.float64) * idf / Nb
        assert abs(R.score(a, Na, b, Nb, idf)[1] - (1.0 - 0.5 * np.abs(va - vb).sum())) < 1e-12


def test_vocabulary_file_layout():
    blob = R.vocabulary_bytes([BC.A, BC.B], [1, 0x0203])
    assert blob == b"ARIABOW\x00" + b"\x01\x00\x00\x00\x02\x00\x00\x00" + bytes(32) + b"\xff" * 32 + b"\x01\x00\x03\x02"


@pytest.fixture(scope="module")
def scene_result():
    train, db, queries = BC.scene()
    words, idf, run = R.train(train, BC.SCENE_WORDS, 10)
    ix = R.BowIndexRef(words, idf, capacity=64, top_k=4, min_frames_between=10)
    for p, v in enumerate(db):
        ix.add(p, v)
    return ix, [ix.query(1000 + p, v) for p, v in enumerate(queries)], run


def test_scene_retrieval_is_40_of_40(scene_result):
    """40 places of 300 random descriptors, a view is 200 of them with 8 flipped bits each; one view per place trains V = 256 for
    10 iterations, a second fills the database, a third queries. Seed 7, the seed of the prototype: the restatement places 40 of
    40 first. The margin (right place over the best wrong one) is printed, not asserted."""
    ix, results, run = scene_result
    right, margin = 0, np.inf
    for p, (hits, count) in enumerate(results):
        assert count >= 2
        right += int(hits["index"][0] == p)
        margin = min(margin, hits["score"][0] / hits["score"][1])
    print("scene: %d of %d top-1, least margin %.3f, %d training iterations" % (right, len(results), margin, run))
    assert right == BC.SCENE_PLACES == len(results)


class _StubBow:
    def __init__(self, hits, count):
        self.hits, self.count = hits, count

    def query_device(self, query_id, d_query, nq):
        return self.hits, self.count


def test_bow_candidates_are_a_subset_of_the_full_scan():
    """find_candidates_bow's host rules on the subset the index names give nothing the full scan's rules would not give, with
    the same scores."""
    rng = np.random.default_rng(5)
    for trial in range(50):
        n, nq, qid, mfb = 40, 200, 60, 30
        good_all = rng.integers(0, 80, n)
        ids, counts = np.arange(n) + rng.integers(0, 25), rng.integers(0, 2, n) * 200
        full = dict(score_candidates(good_all, nq, qid, ids, counts, mfb))
        top = np.sort(rng.choice(n, 10, replace=False))
        rng.shuffle(top)
        hits = np.zeros(12, R.HIT_DTYPE)
        hits["index"] = -1
        hits["index"][:10] = top
        got = R.bow_subset_candidates(hits, 10, good_all[top], nq, qid, ids, counts, mfb)
        assert len(got) <= 5 and [s for _, s in got] == sorted((s for _, s in got), reverse=True)
        everything = {i: float(g) / nq for i, (g, k, c) in enumerate(zip(good_all, ids, counts)) if qid - k >= mfb and c > 0 and g / nq > 0.1}
        for i, s in got:
            assert i in top and everything[i] == s
        if set(full) <= set(top.tolist()):
            assert dict(got) == full
