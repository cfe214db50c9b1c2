"""Case table of the place-recognition stage. Every expected answer is written down from the construction of the case, not computed
by the restatement (aria_slam_amd/bow_ref.py): tests/test_bow_host.py holds the restatement to it, tests/test_bow_kernel_emulation.py
the kernel's plain arithmetic, tests/test_gpu_bow.py the device."""
import numpy as np

ONE = 0x3FF0000000000000          # bit patterns of the fp64 scores the cases are built to give
HALF = 0x3FE0000000000000
QUARTER = 0x3FD0000000000000
THIRD = 0x3FD5555555555555        # 2 / 6 and 4 / 12: the same double
FIVE_SIXTHS = 0x3FEAAAAAAAAAAAAB


def d(*bits):
    """A descriptor with exactly these bits set (bit b = bit b & 7 of byte b >> 3)."""
    out = np.zeros(32, np.uint8)
    for b in bits:
        out[b >> 3] |= 1 << (b & 7)
    return out


A = np.zeros(32, np.uint8)
B = np.full(32, 0xFF, np.uint8)


def numbered(n):
    """n distinct descriptors: descriptor j holds j in its first two bytes and its complement in the next two, so two of them
    differ in at least two bits and each is at distance 0 from itself alone."""
    out = np.zeros((n, 32), np.uint8)
    j = np.arange(n)
    out[:, 0], out[:, 1] = j & 0xFF, j >> 8
    out[:, 2], out[:, 3] = ~(j & 0xFF) & 0xFF, ~(j >> 8) & 0xFF
    return out


def _frames(*lists):
    return [np.array(l, np.uint8).reshape(-1, 32) for l in lists]


# ---- the integer logarithm: (F, n_w, Q8 word). log2(3) = 1.58496...: 256 + floor(0.58496 * 256 = 149.75) = 405;
# log2(65535) = 15.99998: 15 * 256 + 255; log2(65535 / 65534) = 0.000022: 0.
ILOG = [(1, 1, 0), (2, 1, 256), (3, 1, 405), (65535, 1, 4095), (65535, 65534, 0), (4, 1, 512), (6, 2, 405), (65535, 32768, 255)]
# the weight: n_w = 0 and n_w = F give 0
IDF = [(5, 0, 0), (5, 5, 0), (2, 1, 256), (3, 1, 405), (65535, 1, 4095), (65535, 65534, 0)]


def train_cases():
    """name, frames, V, iters -> words, idf_q, iterations run; or refused."""
    n33, n257 = numbered(33), numbered(257)
    return [
        # one word: it starts as descriptor 0 = B; members B, B, A: every bit has 2 ones of 3 -> B again, nothing changed
        dict(name="v1", frames=_frames([B, B, A]), V=1, iters=10, words=[B], idf=[0], run=1),
        # majority tie: two members, bits 0 and 2 have one 1 of two -> 0, bit 1 has two -> 1. The word changes in iteration 1,
        # iteration 2 changes nothing and is the last
        dict(name="majority_tie", frames=_frames([d(0, 1), d(1, 2)]), V=1, iters=10, words=[d(1)], idf=[0], run=2),
        # the same with one iteration allowed: stops after it although the word changed
        dict(name="iters_cap", frames=_frames([d(0, 1), d(1, 2)]), V=1, iters=1, words=[d(1)], idf=[0], run=1),
        # n == V, duplicate initial words: both descriptors go to word 0 (lowest of equals); word 1 has no member and keeps its
        # bits; word 0 is in both frames (n_w = F), word 1 in none (n_w = 0): both weights 0
        dict(name="duplicates_empty_word", frames=_frames([d(5)], [d(5)]), V=2, iters=10, words=[d(5), d(5)], idf=[0, 0], run=1),
        # descriptors A | B A: initial words A (descriptor 0) and B (descriptor floor(1 * 3 / 2) = 1); A is in both frames, B in
        # one of two: log2(2) = 256
        dict(name="idf_two", frames=_frames([A], [B, A]), V=2, iters=10, words=[A, B], idf=[0, 256], run=1),
        # descriptors A | A | B A: word 1 = descriptor floor(1 * 4 / 2) = 2 = B; B is in one frame of three: log2(3) -> 405
        dict(name="idf_three", frames=_frames([A], [A], [B, A]), V=2, iters=10, words=[A, B], idf=[0, 405], run=1),
        # an empty frame counts in F: B in one frame of four: log2(4) = 512; A in three of four: log2(4/3) = 0.415 -> 106
        dict(name="empty_frame", frames=_frames([A], [], [A], [B, A]), V=2, iters=10, words=[A, B], idf=[106, 512], run=1),
        # V not a multiple of the kNN tile, n == V: every descriptor is its own word, one frame: all weights 0
        dict(name="v33", frames=[n33], V=33, iters=10, words=n33, idf=[0] * 33, run=1),
        dict(name="v257", frames=[n257[:100], n257[100:]], V=257, iters=10, words=n257, idf=[256] * 257, run=1),
        dict(name="n_is_v_minus_1", frames=_frames([A, B]), V=3, iters=10, refused=True),
        dict(name="v_zero", frames=_frames([A, B]), V=0, iters=10, refused=True),
        dict(name="v_too_large", frames=[numbered(4097)], V=4097, iters=10, refused=True),
    ]


def transform_cases():
    """name, words, idf, rows (the handle's limit), stride, frames (count, descriptors) -> tf rows, norms, deferred error."""
    def pattern(c):                       # descriptor i of a frame: B when i % 3 == 0, else A
        return np.array([B if i % 3 == 0 else A for i in range(max(c, 0))], np.uint8).reshape(-1, 32)
    counts = [0, 1, 63, 64, 65, 66, 2, -1, 65]
    ok = [c if 0 <= c <= 65 else 0 for c in counts]
    tf = [[c - (c + 2) // 3, (c + 2) // 3] for c in ok]
    n33, n257 = numbered(33), numbered(257)
    w33, w257 = [1 + (w % 7) for w in range(33)], [1 + (w % 7) for w in range(257)]
    return [
        # a descriptor at distance 1 from both words goes to word 0; one at distance 0 from word 1 goes there
        dict(name="equidistant", words=[A, d(0, 1)], idf=[3, 5], rows=8, stride=4, counts=[1, 2, 3],
             frames=_frames([d(0)], [d(0, 1), d(1)], [d(0, 1), d(0, 1), d(7)]), tf=[[1, 0], [1, 1], [1, 2]], norm=[3, 8, 13], error=False),
        # one word takes everything
        dict(name="v1", words=[d(9)], idf=[7], rows=8, stride=4, counts=[3, 0], frames=_frames([A, B, d(9)], []), tf=[[3], [0]],
             norm=[21, 0], error=False),
        # frames of 0, 1, 63, 64 and 65 descriptors; rows + 1 and -1 inside the batch are refused alone and give empty bags
        dict(name="frame_sizes", words=[A, B], idf=[2, 7], rows=65, stride=66, counts=counts, frames=[pattern(min(c, 66)) for c in counts],
             tf=tf, norm=[2 * a + 7 * b for a, b in tf], error=True),
        dict(name="v33", words=n33, idf=w33, rows=64, stride=40, counts=[33, 2], frames=[n33, n33[[32, 32]]],
             tf=[[1] * 33, [0] * 32 + [2]], norm=[sum(w33), 2 * w33[32]], error=False),
        dict(name="v257", words=n257, idf=w257, rows=300, stride=257, counts=[257, 3], frames=[n257, n257[[256, 0, 256]]],
             tf=[[1] * 257, [1] + [0] * 255 + [2]], norm=[sum(w257), w257[0] + 2 * w257[256]], error=False),
    ]


def _hit(index, kid, S, bits):
    return (index, kid, S, bits)


NONE = (-1, -1, 0, 0)


def query_cases():
    """name, V = 4 words with weight 1 each, capacity, top_k, min_frames_between, entries (id, tf), queries (id, tf) ->
    per query (count, hits as (index, id, S, score bits)). The norm of a bag is the sum of its tf here."""
    main = [(0, [1, 2, 0, 0]), (1, [0, 0, 3, 1]), (2, [1, 0, 1, 0]), (3, [0, 0, 0, 0]), (4, [1, 2, 0, 0]), (5, [4, 0, 0, 0])]
    return [
        dict(name="main", capacity=8, top_k=4, mfb=10, entries=main, size=6, info=[(0, 0, 3), (3, 3, 0), (5, 5, 4)], queries=[
            # identical bags (0 and 4): S = 3 * 3 = Nq * Nd, exactly 1.0, lower index first; entry 1 is disjoint and entry 3
            # empty: never returned; entries 2 and 5: S = 2 of 6 and 4 of 12, the same double, lower index first. The gate is
            # inclusive: 15 - 5 = 10 passes
            (15, [1, 2, 0, 0], 4, [_hit(0, 0, 9, ONE), _hit(4, 4, 9, ONE), _hit(2, 2, 2, THIRD), _hit(5, 5, 4, THIRD)]),
            # one less: entry 5 is too recent, K is larger than the candidates, the rest is padding
            (14, [1, 2, 0, 0], 3, [_hit(0, 0, 9, ONE), _hit(4, 4, 9, ONE), _hit(2, 2, 2, THIRD), NONE]),
            # entry 2: S = min(1 * 2, 1 * 2) = 2 of 4: exactly 0.5. Entries 0, 4: S = 2 + 3 = 5 of 6; entry 5: 4 of 8
            (100, [1, 1, 0, 0], 4, [_hit(0, 0, 5, FIVE_SIXTHS), _hit(4, 4, 5, FIVE_SIXTHS), _hit(2, 2, 2, HALF), _hit(5, 5, 4, HALF)]),
            # entry 5: S = min(1 * 4, 4 * 4) = 4 of 16: exactly 0.25, and pushed out by four entries at 0.5
            (100, [1, 1, 1, 1], 4, [_hit(0, 0, 6, HALF), _hit(1, 1, 8, HALF), _hit(2, 2, 4, HALF), _hit(4, 4, 6, HALF)]),
            (100, [0, 0, 0, 4], 1, [_hit(1, 1, 4, QUARTER), NONE, NONE, NONE]),
            # an empty query
            (100, [0, 0, 0, 0], 0, [NONE, NONE, NONE, NONE]),
            # nothing old enough
            (9, [1, 2, 0, 0], 0, [NONE, NONE, NONE, NONE]),
        ]),
        # capacity 4, five entries: id 0 is dropped and every index shifts down by one
        dict(name="drop", capacity=4, top_k=4, mfb=0, size=4, info=[(0, 1, 1), (3, 4, 2)],
             entries=[(0, [1, 0, 0, 0]), (1, [0, 1, 0, 0]), (2, [0, 0, 1, 0]), (3, [0, 0, 0, 1]), (4, [1, 1, 0, 0])], queries=[
            (100, [0, 1, 0, 0], 2, [_hit(0, 1, 1, ONE), _hit(3, 4, 1, HALF), NONE, NONE]),
            (100, [1, 0, 0, 0], 1, [_hit(3, 4, 1, HALF), NONE, NONE, NONE]),
        ]),
        dict(name="empty_database", capacity=4, top_k=2, mfb=0, size=0, info=[], entries=[], queries=[(7, [1, 0, 0, 0], 0, [NONE, NONE])]),
    ]


QUERY_WORDS = [d(0, 1, 2, 3), d(60, 61, 62, 63), d(120, 121, 122, 123), d(200, 201, 202, 203)]      # any four distinct words
QUERY_IDF = [1, 1, 1, 1]


def expected_hits(hits):
    """The (index, id, S, score bits) tuples of a case as records of bow_ref.HIT_DTYPE."""
    from aria_slam_amd.bow_ref import HIT_DTYPE
    out = np.zeros(len(hits), HIT_DTYPE)
    for k, (i, kid, S, bits) in enumerate(hits):
        out[k] = (i, 0, kid, S, 0.0)
    out["score"] = np.array([h[3] for h in hits], np.uint64).view(np.float64)
    return out


# ---- the generated scene: 40 places of 300 random descriptors; a view is 200 of them with 8 flipped bits each -------------
SCENE_SEED = 7
SCENE_PLACES, SCENE_POINTS, SCENE_VIEW, SCENE_FLIPS, SCENE_WORDS = 40, 300, 200, 8, 256


def scene(seed=SCENE_SEED):
    """(train views, database views, query views): three lists of 40 [200, 32] uint8 arrays."""
    rng = np.random.default_rng(seed)
    places = rng.integers(0, 256, (SCENE_PLACES, SCENE_POINTS, 32), dtype=np.uint8)

    def view(p):
        v = places[p][rng.choice(SCENE_POINTS, SCENE_VIEW, replace=False)].copy()
        for row in v:
            for b in rng.choice(256, SCENE_FLIPS, replace=False):
                row[b >> 3] ^= 1 << (b & 7)
        return v
    return tuple([view(p) for p in range(SCENE_PLACES)] for _ in range(3))


# ---- the edge groups: every tile, ring position, chunk and size of the query path, the bit budget, transform and training at size.
# A group is a configuration and a list of steps on one index; every expected answer is written from the construction with plain
# integers and one IEEE division, never by the restatement. tests/test_bow_edges_host.py holds the restatement to them and counts
# what they reach, tests/test_gpu_bow_edges.py the device.
LADDER_BEST = [299, 64, 0, 191, 128, 63, 256, 255]     # index of rank 0, 1, ..: four waves, five tiles, both trips of a thread
LADDER_SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320]
LADDER_QID = 10 ** 6
RING_CAPACITIES = [1, 100, 256, 257, 300]
RING_CALLS = [1, 255, 256, 257, 600]
RING_HEADS = [1, 63, 64, 65, 319]
EDGE_V = [1, 7, 8, 9, 33, 257, 511, 512, 513, 520, 1024, 2047, 2048, 2049, 2056, 4095, 4096]
TWO_POW_24 = 1 << 24


def _bits(num, den):
    """The bit pattern of the one division double(num) / double(den); both are exact doubles (below 2^53)."""
    assert 0 < num < 2 ** 53 and 0 < den < 2 ** 53
    return int((np.float64(num) / np.float64(den)).view(np.uint64))


def ladder_perm():
    """perm[e] = the rank of ladder entry e, a permutation of 0 .. 319: ranks 0 .. 7 at LADDER_BEST, the rest in the order of
    (131 e) mod 321 (131 and 321 are coprime, so no two indices share a key)."""
    perm = [-1] * 320
    for r, e in enumerate(LADDER_BEST):
        perm[e] = r
    rest = sorted((e for e in range(320) if perm[e] < 0), key=lambda e: (131 * e) % 321)
    for k, e in enumerate(rest):
        perm[e] = 8 + k
    return perm


def ladder_bags(ranks):
    """V = 2, weights [1, 1]: the entry of rank r is the bag [1, r] with norm 1 + r. -> (tf [n, 2] uint16, norm [n] int32)."""
    tf = np.array([[1, r] for r in ranks], np.uint16).reshape(-1, 2)
    return tf, np.array([1 + r for r in ranks], np.int32)


def ladder_hits(db, K, a=1, admitted=None):
    """The query [a, 0] (norm a) against ladder entries db = [(id, rank)], oldest first: against rank r, S = min(a (1 + r), a) = a
    and the score is a / (a (1 + r)). The K smallest ranks among the admitted, equal ranks to the lower index.
    -> (count, K hit tuples)."""
    cand = sorted((r, i) for i, (kid, r) in enumerate(db) if admitted is None or admitted(i, kid))[:K]
    hits = [_hit(i, db[i][0], a, _bits(a, a * (1 + r))) for r, i in cand]
    return len(hits), hits + [NONE] * (K - len(hits))


def _add(ids, ranks, error=False):
    tf, norm = ladder_bags(ranks)
    return dict(op="add", tf=tf, norm=norm, ids=list(ids), error=error)


def _ladder_query(db, K, qids=(LADDER_QID,), a=None, admitted=None, sample=(0,)):
    a = [1] * len(qids) if a is None else list(a)
    want = [ladder_hits(db, K, a[j], None if admitted is None else (lambda i, kid, q=q: admitted(q, i, kid))) for j, q in enumerate(qids)]
    return dict(op="query", tf=np.array([[x, 0] for x in a], np.uint16), norm=np.array(a, np.int32), qids=list(qids),
                counts=[w[0] for w in want], hits=[w[1] for w in want], error=False, sample=list(sample))


def _index_group(name, capacity, top_k, mfb, steps, V=2, idf=(1, 1)):
    return dict(name=name, kind="index", V=V, words=numbered(V), idf=np.array(idf, np.uint16), rows=16, capacity=capacity,
                top_k=top_k, mfb=mfb, steps=steps)


def _groups_a():
    perm = ladder_perm()
    out = []
    # sizes: one index grows through every size on both sides of 64, 128 and 256 and is asked at each
    steps, have = [], 0
    for n in LADDER_SIZES:
        steps.append(_add([10 * e for e in range(have, n)], perm[have:n]))
        have = n
        steps.append(dict(op="state", size=n, info=[(0, 0, 1 + perm[0]), (n - 1, 10 * (n - 1), 1 + perm[n - 1])]))
        steps.append(_ladder_query([(10 * e, perm[e]) for e in range(n)], 8))
    out.append(_index_group("A ladder sizes", 320, 8, 0, steps))
    # ties: 5 and 261 (one thread, two trips), 70 and 130 (two waves), 63 and 64 (neighbouring waves and tiles); every other
    # entry is worse and distinct. K = 5 cuts the last pair: 63 is returned, 64 is not
    ranks = [20 + e for e in range(300)]
    for r, pair in enumerate([(5, 261), (70, 130), (63, 64)]):
        for e in pair:
            ranks[e] = r
    db = [(10 * e, ranks[e]) for e in range(300)]
    q = _ladder_query(db, 5)
    assert [h[0] for h in q["hits"][0]] == [5, 261, 70, 130, 63]
    out.append(_index_group("A ladder ties", 320, 5, 0, [_add([k for k, _ in db], ranks), q]))
    # the same ties one place later: K = 6 ends on the pair, K = 3 cuts the pair of two waves
    for K, want in ((6, [5, 261, 70, 130, 63, 64]), (3, [5, 261, 70])):
        q = _ladder_query(db, K)
        assert [h[0] for h in q["hits"][0]] == want
        out.append(_index_group("A ladder ties K=%d" % K, 300, K, 0, [_add([k for k, _ in db], ranks), q]))
    # K = 32 with 1, 31, 32, 33 and 300 candidates; K = 1 with the best entry last
    steps, have = [], 0
    for n in (1, 31, 32, 33, 300):
        steps.append(_add([10 * e for e in range(have, n)], perm[have:n]))
        have = n
        steps.append(_ladder_query([(10 * e, perm[e]) for e in range(n)], 32))
    assert [s["counts"] for s in steps[1::2]] == [[1], [31], [32], [32], [32]] and steps[-1]["hits"][0][0][0] == 299
    out.append(_index_group("A ladder K=32", 320, 32, 0, steps))
    q = _ladder_query([(10 * e, perm[e]) for e in range(300)], 1)
    assert q["hits"][0] == [_hit(299, 2990, 1, ONE)]
    out.append(_index_group("A ladder K=1", 300, 1, 0, [_add([10 * e for e in range(300)], perm[:300]), q]))
    return out


def ring_rank(t):
    """The rank of the t-th bag a ring group adds, t < 1373 (a prime): distinct, and neither rising nor falling with t."""
    return (577 * t) % 1373


def _groups_b():
    perm = ladder_perm()
    out = []
    for c in RING_CAPACITIES:
        steps, total = [], 0
        for n in RING_CALLS:                   # one call each, onto the ring as the calls before left it
            steps.append(_add([7 * t - 3 for t in range(total, total + n)], [ring_rank(t) for t in range(total, total + n)]))
            total += n
            size = min(total, c)
            first = total - size               # the oldest survivor; bag t lies in slot t mod c, so slot c - 1 is index wrap
            wrap = c - 1 - first % c
            at = sorted(set(i for i in (0, 1, size - 1, wrap, wrap + 1) if 0 <= i < size))
            steps.append(dict(op="state", size=size, info=[(i, 7 * (first + i) - 3, 1 + ring_rank(first + i)) for i in at]))
            steps.append(_ladder_query([(7 * t - 3, ring_rank(t)) for t in range(first, total)], 8))
        out.append(_index_group("B ring capacity=%d" % c, c, 8, 0, steps))
    # head = h on the ladder's capacity: h bags that score 1.0 and must be gone, then the ladder; the size-320 query of group A
    for h in RING_HEADS:
        steps = [_add([-7] * h + [10 * e for e in range(320)], [0] * h + perm),
                 dict(op="state", size=320, info=[(0, 0, 1 + perm[0]), (319 - h, 10 * (319 - h), 1 + perm[319 - h]),
                                                  (320 - h, 10 * (320 - h), 1 + perm[320 - h]), (319, 3190, 1 + perm[319])]),
                 _ladder_query([(10 * e, perm[e]) for e in range(320)], 8)]
        out.append(_index_group("B ring head=%d" % h, 320, 8, 0, steps))
    return out


def gate_query_id(j):
    """Query j of group C admits the entries e <= m (ids 10 e, gate 30): 29 admits none, 30 exactly entry 0 by a difference of
    exactly 30; from j = 2 on m = 89 j mod 300 with a difference of exactly 30, 39 or 35 at entry m."""
    if j < 2:
        return 29 + j
    return 30 + 10 * ((89 * j) % 300) + (0, 9, 5)[j % 3]


def _groups_c():
    perm = ladder_perm()
    db = [(10 * e, perm[e]) for e in range(300)]
    add = _add([k for k, _ in db], perm[:300])
    steps = [add]
    for n in (257, 261):
        qids = [gate_query_id(j) for j in range(n)]
        q = _ladder_query(db, 8, qids, a=[1 + j % 5 for j in range(n)], admitted=lambda q_, i, kid: q_ - kid >= 30,
                          sample=(0, 1, 2, 255, 256, n - 1))
        assert q["counts"][0] == 0 and q["counts"][1] == 1 and q["hits"][1][0][:2] == (0, 0)
        if n == 261:
            # bag 130 is empty (norm 0, no error); bag 258's norm is one more than its weighted counts (refused, an error)
            q["tf"][130] = [0, 0]
            q["norm"][130] = 0
            q["norm"][258] += 1
            for j in (130, 258):
                q["counts"][j], q["hits"][j] = 0, [NONE] * 8
            q["error"] = True
            q["sample"] = [129, 130, 131, 256, 257, 259, 260]
        steps.append(q)
    out = [_index_group("C query chunks", 300, 8, 30, steps)]
    # ids: negative, around +-2^40, a difference of exactly the gate, a query older than every entry
    T = 1 << 40
    ids, ranks = [-T - 5, -T, -7, T - 30, T, T + 1], [3, 1, 4, 0, 2, 5]
    db = list(zip(ids, ranks))
    qids = [T, -T + 30, 23, -2 * T, T + 31, -T + 29]
    q = _ladder_query(db, 4, qids, admitted=lambda q_, i, kid: q_ - kid >= 30, sample=range(6))
    assert [[h[0] for h in hs] for hs in q["hits"]] == [[3, 1, 0, 2], [1, 0, -1, -1], [1, 0, 2, -1], [-1] * 4, [3, 1, 4, 0], [0, -1, -1, -1]]
    out.append(_index_group("C ids gate=30", 16, 4, 30, [_add(ids, ranks), q]))
    db = [(-3, 1), (6, 0)]
    q = _ladder_query(db, 4, [-4, -3, 5, 6], admitted=lambda q_, i, kid: q_ - kid >= 0, sample=range(4))
    assert q["counts"] == [0, 1, 1, 2]
    out.append(_index_group("C ids gate=0", 16, 4, 0, [_add([-3, 6], [1, 0]), q]))
    return out


# group D, second half: weights [4095, 4094], the query [2048, 2047] against the entries [2049, 2048] and [2048, 2046]. Per word
# (v Nd, u Nq): the query's product and the entry's. Against entry 0 the two differ by 4095 * 4094 = 16764930 < 2^24 on both words.
D_Q = dict(tf=[2048, 2047], v=(8386560, 8380418), N=16766978)
D_E = [dict(tf=[2049, 2048], u=(8390655, 8384512), N=16775167,
            products=[(140685944555520, 140685927790590), (140582911479806, 140582928244736)], smaller=["entry", "query"],
            S=281268839270396, NN=281268856035326),
       dict(tf=[2048, 2046], u=(8386560, 8376324), N=16762884,
            products=[(140582932439040, 140617267015680), (140479974805512, 140445640228872)], smaller=["query", "entry"],
            S=281028572667912, NN=281062907244552)]


def _groups_d():
    M = TWO_POW_24 - 1                                   # 4097 * 4095: the largest norm there is
    # weights [4095, 1]. Entries: [4097, 0] (N = 2^24 - 1, accepted), [4096, 4096] (N = 2^24 exactly), [65535, 0] (a weighted
    # count above 2^24, its true norm given), [1, 0] with a negative norm, [1, 1] (N = 4096, accepted). The three in the middle are
    # stored empty; one deferred error for the call
    tf = np.array([[4097, 0], [4096, 4096], [65535, 0], [1, 0], [1, 1]], np.uint16)
    norm = np.array([M, TWO_POW_24, 65535 * 4095, -4095, 4096], np.int32)
    ids = [0, 1, 2, 3, 4]
    add = dict(op="add", tf=tf, norm=norm, ids=ids, error=True)
    state = dict(op="state", size=5, info=[(0, 0, M), (1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 4, 4096)])
    # the same five as queries. [4097, 0] against itself: S = M^2, 1.0; against [1, 1]: S = min(M * 4096, 4095 * M) = 4095 M.
    # [1, 1] against [4097, 0]: S = min(4095 M, M * 4096) + min(1 * M, 0) = 4095 M; against itself 4096^2
    hits = [[_hit(0, 0, M * M, ONE), _hit(4, 4, 4095 * M, _bits(4095 * M, M * 4096)), NONE, NONE], [NONE] * 4, [NONE] * 4, [NONE] * 4,
            [_hit(4, 4, 4096 * 4096, ONE), _hit(0, 0, 4095 * M, _bits(4095 * M, 4096 * M)), NONE, NONE]]
    query = dict(op="query", tf=tf.copy(), norm=norm.copy(), qids=[9] * 5, counts=[2, 0, 0, 0, 2], hits=hits, error=True, sample=[0, 4])
    out = [_index_group("D norm bound", 8, 4, 0, [add, state, query], idf=(4095, 1))]
    # the accepted bags alone raise no error, as entries or as queries
    ok = [0, 4]
    out.append(_index_group("D norm bound clean", 8, 4, 0, [
        dict(op="add", tf=tf[ok], norm=norm[ok], ids=[0, 4], error=False),
        dict(op="query", tf=tf[ok], norm=norm[ok], qids=[9, 9], counts=[2, 2], error=False, sample=[0, 1],
             hits=[[_hit(0, 0, M * M, ONE), _hit(1, 4, 4095 * M, _bits(4095 * M, M * 4096)), NONE, NONE],
                   [_hit(1, 4, 4096 * 4096, ONE), _hit(0, 0, 4095 * M, _bits(4095 * M, 4096 * M)), NONE, NONE]])], idf=(4095, 1)))
    # 48-bit products decided below bit 24
    for e in D_E:
        assert e["S"] == sum(min(p) for p in e["products"]) and e["NN"] == D_Q["N"] * e["N"]
        assert [("query" if a < b else "entry") for a, b in e["products"]] == e["smaller"]
    want = sorted(range(2), key=lambda i: (-_bits(D_E[i]["S"], D_E[i]["NN"]), i))
    hits = [[_hit(i, 50 + i, D_E[i]["S"], _bits(D_E[i]["S"], D_E[i]["NN"])) for i in want] + [NONE, NONE]]
    out.append(_index_group("D products", 8, 4, 0, [
        dict(op="add", tf=np.array([e["tf"] for e in D_E], np.uint16), norm=np.array([e["N"] for e in D_E], np.int32), ids=[50, 51], error=False),
        dict(op="query", tf=np.array([D_Q["tf"]], np.uint16), norm=np.array([D_Q["N"]], np.int32), qids=[99], counts=[2], hits=hits,
             error=False, sample=[0])], idf=(4095, 4094)))
    return out


def probe_words(V):
    return sorted(set(w for w in (0, 7, 8, 511, 512, 519, 520, 2047, 2048, 2055, 2056, V - 8, V - 1) if 0 <= w < V))


def _groups_e():
    out = []
    for V in EDGE_V:
        P = probe_words(V)
        n = len(P)
        wt = [2 * k + 1 for k in range(n)]
        N = sum(wt)                                      # = n^2
        idf = np.zeros(V, np.uint16)
        idf[P] = wt
        tf = np.zeros((1 + n, V), np.uint16)             # bag 0: every probe word once; bag 1 + k: probe word k alone
        tf[0, P] = 1
        for k, w in enumerate(P):
            tf[1 + k, w] = 1
        norm = np.array([N] + wt, np.int32)
        ids = list(range(100, 101 + n))
        # the full bag: against entry 0 S = N^2; against entry 1 + k the one shared word gives min(wt N', ..) with both norms:
        # min(wt_k * wt_k, wt_k * N) = wt_k^2 of N wt_k. A single bag k: the same S against entry 0, wt_k^2 of wt_k^2 against its own
        def rank(c):
            c.sort(key=lambda h: (-h[3], h[0]))
            return c + [NONE] * (16 - len(c))
        hits = [rank([_hit(0, 100, N * N, ONE)] + [_hit(1 + k, 101 + k, wt[k] ** 2, _bits(wt[k] ** 2, N * wt[k])) for k in range(n)])]
        for k in range(n):
            hits.append(rank([_hit(0, 100, wt[k] ** 2, _bits(wt[k] ** 2, wt[k] * N)), _hit(1 + k, 101 + k, wt[k] ** 2, ONE)]))
        steps = [dict(op="add", tf=tf, norm=norm, ids=ids, error=False),
                 dict(op="query", tf=tf.copy(), norm=norm.copy(), qids=[10 ** 4] * (1 + n), counts=[1 + n] + [2] * n, hits=hits, error=False,
                      sample=[0, 1, n])]
        out.append(_index_group("E V=%d" % V, 16, 16, 0, steps, V=V, idf=idf))
    return out


F_ROWS = 4096
F_FRAMES = 300
F_REFUSED = {260: -1, 270: F_ROWS + 1}
F_ONE_WORD, F_EVERY_WORD = 280, 290


def _group_f_transform():
    """V = 4096 words numbered(4096), so a descriptor equal to word w is on word w. Weight 1 + w mod 7, word 4095: 4095. Frame f
    holds f mod 5 descriptors, descriptor i on word (13 f + 7 i) mod 4096, except the four named frames."""
    V = 4096
    words = numbered(V)
    idf = np.array([1 + w % 7 for w in range(V)], np.uint16)
    idf[4095] = 4095
    frames, counts, tf, norm = [], [], np.zeros((F_FRAMES, V), np.uint16), []
    for f in range(F_FRAMES):
        if f in F_REFUSED:
            on, c = [5, 6, 7], F_REFUSED[f]              # descriptors are there; the count is refused and the bag is empty
        elif f == F_ONE_WORD:
            on, c = [4095] * F_ROWS, F_ROWS
        elif f == F_EVERY_WORD:
            on, c = [(w * 5) % V for w in range(V)], F_ROWS      # every word once, not in order
        else:
            on = [(13 * f + 7 * i) % V for i in range(f % 5)]
            c = len(on)
        frames.append(words[on])
        counts.append(c)
        if f not in F_REFUSED:
            for w in on:
                tf[f, w] += 1
        norm.append(sum(int(tf[f, w]) * int(idf[w]) for w in set(on)) if f not in F_REFUSED else 0)
    assert tf[F_ONE_WORD, 4095] == 4096 and norm[F_ONE_WORD] == 4096 * 4095 and (tf[F_EVERY_WORD] == 1).all()
    assert norm[F_EVERY_WORD] == int(idf.astype(np.int64).sum())
    return dict(name="F transform V=4096", kind="transform", V=V, words=words, idf=idf, rows=F_ROWS, stride=F_ROWS, frames=frames,
                counts=counts, tf=tf, norm=norm, error=True, sample=[0, 4, 259, 260, 270, F_ONE_WORD, F_EVERY_WORD, 299])


def _flip(D, rng, most):
    for row in D:
        for b in rng.choice(256, int(rng.integers(0, most + 1)), replace=False):
            row[b >> 3] ^= 1 << (b & 7)


def _groups_f_train():
    """Training sets; bow_ref.train is their answer (no closed form). V = 4096: 30 frames of 400 descriptors from 200 seeds with
    up to three flipped bits; the first 24 descriptors of every frame are seed 0, twelve of them exact, so one word gathers more
    than 256 members and the initial words that repeat it get none. V = 33: 300 frames of 0 to 3 descriptors; from frame 256 on
    every other frame is empty."""
    rng = np.random.default_rng(23)
    seeds = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    big = []
    for f in range(30):
        pick = rng.integers(0, 200, 400)
        pick[:24] = 0
        D = seeds[pick].copy()
        _flip(D[12:], rng, 3)
        big.append(D)
    rng = np.random.default_rng(29)
    seeds = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    small = []
    for f in range(300):
        n = 0 if (f >= 256 and f % 2 == 0) else int(rng.integers(0, 4))
        D = seeds[rng.integers(0, 40, n)].copy().reshape(-1, 32)
        _flip(D, rng, 2)
        small.append(D)
    return [dict(name="F train V=4096", kind="train", V=4096, iters=3, frames=big),
            dict(name="F train V=33", kind="train", V=33, iters=10, frames=small)]


def edge_groups():
    """Every group, A to F (see the comment above LADDER_BEST)."""
    return _groups_a() + _groups_b() + _groups_c() + _groups_d() + _groups_e() + [_group_f_transform()] + _groups_f_train()
