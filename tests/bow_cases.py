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
