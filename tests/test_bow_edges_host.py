"""The edge groups of the place-recognition stage (tests/bow_cases.py, edge_groups()) on the CPU: the definition
(aria_slam_amd/bow_ref.py) held to every answer written down from the constructions and to a brute-force double loop in plain
Python integers; the kernel's plain arithmetic, compiled for the host by tests/test_bow_kernel_emulation.py, held to the answers of
groups D and E; the census of what the groups reach (sizes around 64, 128 and 256, ring heads with a tile across the wrap, chunk
counts, probe words, product magnitudes, the training sets); and wrong copies of the definition, each of which the groups notice
and most of which the case table before them (query_cases and the scene) does not. Run with -s for the census and the table of
wrong copies. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_cases as BC   # noqa: E402
from aria_slam_amd import bow_ref as R   # noqa: E402
from test_bow_kernel_emulation import emu   # noqa: E402,F401  (the one host build of the kernel's plain arithmetic)

GROUPS = BC.edge_groups()
INDEX = [g for g in GROUPS if g["kind"] == "index"]
BY_NAME = {g["name"]: g for g in GROUPS}
assert len(BY_NAME) == len(GROUPS)


def _i32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


class Copy:
    """Rules 5 to 8 as a double loop over entries and words in Python integers, with one division. `wrong` names one mistake;
    without one this is the definition (asserted against bow_ref on the old table and on every group)."""

    def __init__(self, idf, capacity, top_k, mfb, wrong=None):
        self.idf, self.cap, self.K, self.mfb, self.wrong = [int(x) for x in idf], capacity, top_k, mfb, wrong
        self.db = []

    def held(self, tf, norm):
        N = sum(int(t) * w for t, w in zip(tf, self.idf))
        limit = BC.TWO_POW_24 + 1 if self.wrong == "the bound N <= 2^24" else BC.TWO_POW_24
        ok = 0 <= int(norm) == N < limit
        return (int(norm) if ok else 0), ok

    def add(self, ids, tf, norm):
        error = False
        for kid, t, n in zip(ids, tf, norm):
            n, ok = self.held(t, n)
            error |= not ok
            if len(self.db) == self.cap:
                if self.wrong == "the ring dropping the newest":
                    continue
                self.db.pop(0)
            self.db.append((int(kid), [int(x) for x in t], n))
        return error

    def term(self, v, n_d, u, n_q):
        if self.wrong == "factors masked to 20 bits":
            v, n_d, u, n_q = (x & 0xFFFFF for x in (v, n_d, u, n_q))
        a, b = v * n_d, u * n_q
        if self.wrong == "products kept in 32 bits":
            a, b = a & 0xFFFFFFFF, b & 0xFFFFFFFF
        return min(a, b)

    def numerator(self, tfs, j, n_q, e, n_d):
        tf_q, tf_d, V = tfs[j], self.db[e][1], len(self.idf)
        S = 0
        for w in range(V):
            if tf_q[w] and not (self.wrong == "words at or beyond 2048 dropped" and w >= 2048):
                S += self.term(int(tf_q[w]) * self.idf[w], n_d, tf_d[w] * self.idf[w], n_q)
        if self.wrong == "padding words read from the next row":
            # the words V .. roundup(V, 8) - 1 of a row are the first words of the row after it, in the queries and in the ring
            nxt_q = tfs[j + 1] if j + 1 < len(tfs) else [0] * V
            nxt_d = self.db[e + 1][1] if e + 1 < len(self.db) else [0] * V
            for p in range(min(-V % 8, V)):
                S += self.term(int(nxt_q[p]) * self.idf[p], n_d, nxt_d[p] * self.idf[p], n_q)
        return S

    def query(self, qids, tf, norm):
        hits, counts, error = [], [], False
        for j, (qid, t, n) in enumerate(zip(qids, tf, norm)):
            n_q, ok = self.held(t, n)
            error |= not ok
            if self.wrong == "the second chunk answered with the first chunk's ids" and j >= 256:
                qid = qids[j - 256]
            cand = []
            for e, (kid, _, n_d) in enumerate(self.db):
                if self.wrong == "only the first 64 entries scored" and e >= 64:
                    break
                if self.wrong == "only the first 256 entries ranked" and e >= 256:
                    break
                diff = int(qid) - kid
                if self.wrong == "id difference in 32 bits":
                    diff = _i32(diff)
                gate = diff > self.mfb if self.wrong == "gate > instead of >=" else diff >= self.mfb
                if n_q <= 0 or n_d <= 0 or not gate:
                    continue
                S = self.numerator(tf, j, n_q, e, n_d)
                if S > 0:
                    cand.append((e, kid, S, BC._bits(S, n_q * n_d)))
            sign = -1 if self.wrong == "ties to the higher index" else 1
            cand.sort(key=lambda c: (-c[3], sign * c[0]))
            cand = cand[:self.K]
            counts.append(len(cand))
            hits.append(cand + [BC.NONE] * (self.K - len(cand)))
        return hits, counts, error


class Ref:
    """bow_ref behind the same three calls."""

    def __init__(self, g):
        self.ix = R.BowIndexRef(g["words"], g["idf"], g["capacity"], g["top_k"], g["mfb"])
        self.idf = g["idf"]

    def add(self, ids, tf, norm):
        error = False
        for kid, t, n in zip(ids, tf, norm):
            n, ok = R.held_norm(t, n, self.idf)
            error |= not ok
            self.ix.add_bag(kid, t, n)
        return error

    def query(self, qids, tf, norm):
        hits, counts, error = [], [], False
        for qid, t, n in zip(qids, tf, norm):
            n, ok = R.held_norm(t, n, self.idf)
            error |= not ok
            h, c = self.ix.query_bag(qid, t, n)
            hits.append(h)
            counts.append(c)
        return hits, counts, error


def _as_bytes(hits):
    return b"".join(h.tobytes() if isinstance(h, np.ndarray) else BC.expected_hits(h).tobytes() for h in hits)


def differences(g, ix, size=None, info=None):
    """Run a group's steps on an index; the list of (step number, what differs from the written answers)."""
    out = []
    for k, s in enumerate(g["steps"]):
        if s["op"] == "add":
            if ix.add(s["ids"], s["tf"], s["norm"]) != s["error"]:
                out.append((k, "add error"))
        elif s["op"] == "state":
            if size(ix) != s["size"]:
                out.append((k, "size"))
            elif [info(ix, i) for i, _, _ in s["info"]] != [(kid, n) for _, kid, n in s["info"]]:
                out.append((k, "info"))
        else:
            hits, counts, error = ix.query(s["qids"], s["tf"], s["norm"])
            if error != s["error"]:
                out.append((k, "query error"))
            if list(counts) != s["counts"]:
                out.append((k, "counts"))
            if _as_bytes(hits) != _as_bytes(s["hits"]):
                out.append((k, "hits"))
    return out


def _copy_of(g, wrong=None):
    return Copy(g["idf"], g["capacity"], g["top_k"], g["mfb"], wrong)


def _copy_differences(g, wrong=None):
    return differences(g, _copy_of(g, wrong), size=lambda ix: len(ix.db), info=lambda ix, i: (ix.db[i][0], ix.db[i][2]))


@pytest.mark.parametrize("g", INDEX, ids=lambda g: g["name"])
def test_the_definition_gives_every_written_answer(g):
    assert differences(g, Ref(g), size=lambda r: r.ix.size(), info=lambda r, i: r.ix.info(i)) == []


@pytest.mark.parametrize("g", INDEX, ids=lambda g: g["name"])
def test_the_double_loop_gives_every_written_answer(g):
    assert _copy_differences(g) == []


def test_ladder_scores_are_distinct_and_falling():
    bits = [BC._bits(1, 1 + r) for r in range(1373)]
    assert all(a > b for a, b in zip(bits, bits[1:]))
    assert sorted(BC.ladder_perm()) == list(range(320)) and [BC.ladder_perm()[e] for e in BC.LADDER_BEST] == list(range(8))
    assert len(set(e % 256 // 64 for e in BC.LADDER_BEST)) == 4 and len(set(e // 64 for e in BC.LADDER_BEST)) == 5
    assert any(e >= 256 for e in BC.LADDER_BEST[:2])                         # the best hit needs the second trip
    assert len(set(BC.ring_rank(t) for t in range(sum(BC.RING_CALLS)))) == sum(BC.RING_CALLS) < 1373
    # a query [a, 0] gives the double of [1, 0]: a / (a (1 + r)) and 1 / (1 + r) are one rational
    assert all(BC._bits(a, a * (1 + r)) == BC._bits(1, 1 + r) for a in range(1, 6) for r in range(400))


# ---- the census ---------------------------------------------------------------------------------------------------------
def _walk(g):
    """Per query step of an index group: (entries, head, capacity, queries); per add step: bags, chunks of the add."""
    total, cap, queries, adds = 0, g["capacity"], [], []
    for s in g["steps"]:
        if s["op"] == "add":
            n, at, chunks = len(s["ids"]), 0, 0
            while at < n:
                at += min(n - at, 256, cap)
                chunks += 1
            wraps = total % cap + min(n, 256, cap) > cap or (n > min(256, cap) and cap % min(256, cap) != 0)
            adds.append((n, chunks, wraps))
            total += n
        elif s["op"] == "query":
            size = min(total, cap)
            queries.append((size, (total - size) % cap, cap, len(s["qids"])))
    return queries, adds


def test_census_of_sizes_heads_and_chunks():
    sizes, heads, add_chunks, query_chunks, wrapping, last_tiles, K_over, aligned = set(), set(), set(), set(), 0, set(), set(), set()
    for g in INDEX:
        queries, adds = _walk(g)
        for size, head, cap, nq in queries:
            sizes.add(size)
            query_chunks.add(-(-nq // 256))
            last_tiles.add((nq % 256) % 4 if nq > 256 else 0)
            tile_over_wrap = any((head + 64 * t) % cap < cap <= (head + 64 * t) % cap + min(64, size - 64 * t) - 1 for t in range(-(-size // 64)))
            if head and g["V"] == 2:
                (heads if tile_over_wrap else aligned).add((cap, head))
        for n, chunks, wraps in adds:
            add_chunks.add(chunks)
            wrapping += wraps
        for s in g["steps"]:
            if s["op"] == "query":
                K_over |= set(g["top_k"] - c for c in s["counts"])
    print("\nsizes asked:", sorted(sizes))
    print("(capacity, head) with a 64-entry tile across the wrap:", sorted(heads))
    print("(capacity, head) with the wrap between two tiles:", sorted(aligned))
    print("chunks per add call:", sorted(add_chunks), " add calls with a chunk over the wrap: %d" % wrapping)
    print("chunks per query call:", sorted(query_chunks), " live queries of a last tile in a second chunk:", sorted(last_tiles - {0}))
    print("top_k minus hits:", sorted(K_over))
    for edge in (64, 128, 256):
        assert {edge - 1, edge, edge + 1} <= sizes
    assert {1, 31, 32, 33, 300, 320} <= sizes
    # head = 64 on capacity 320 is the control: the wrap falls between two tiles
    assert {(320, h) for h in BC.RING_HEADS if h != 64} <= heads and (320, 64) in aligned and any(cap == 300 for cap, _ in heads)
    assert {1, 2, 3, 600} <= add_chunks and wrapping >= 5 and {1, 2} <= query_chunks and 1 in last_tiles
    assert {0, 1, 8, 31} <= K_over and max(g["top_k"] for g in INDEX) == R.MAX_TOP_K
    assert min(g["capacity"] for g in INDEX) == 1 and any(len(s["ids"]) > g["capacity"] for g in INDEX for s in g["steps"] if s["op"] == "add")


def test_census_of_probe_words():
    seen = {}
    for V in BC.EDGE_V:
        g = BY_NAME["E V=%d" % V]
        P = BC.probe_words(V)
        assert P == sorted(set(P)) and P[0] == 0 and P[-1] == V - 1 and all(0 <= w < V for w in P) and len(P) <= 13
        assert [int(x) for x in g["idf"][P]] == [2 * k + 1 for k in range(len(P))] and int(g["idf"].astype(np.int64).sum()) == len(P) ** 2
        tf = g["steps"][0]["tf"]
        assert (tf[0][P] == 1).all() and int(tf[0].sum()) == len(P) and all(tf[1 + k][w] == 1 and tf[1 + k].sum() == 1 for k, w in enumerate(P))
        seen[V] = P
    print("\nprobe words per V:", seen)
    assert seen[4096] == [0, 7, 8, 511, 512, 519, 520, 2047, 2048, 2055, 2056, 4088, 4095]
    assert sum(1 for V in BC.EDGE_V if V % 8) == 10                                          # row strides that are not V
    assert any(512 < -(-V // 8) * 8 < 2048 for V in BC.EDGE_V) and any(-(-V // 8) * 8 > 2048 for V in BC.EDGE_V)


def test_census_of_product_magnitudes():
    """Group D: a pair of 48-bit products above 2^44 that differ below bit 24, on a word where the entry's is the smaller and on
    one where the query's is; and the norms on both sides of the bound."""
    q, close, entry_smaller, query_smaller = BC.D_Q, 0, 0, 0
    assert q["v"] == (2048 * 4095, 2047 * 4094) and q["N"] == sum(q["v"]) < BC.TWO_POW_24
    for e in BC.D_E:
        assert e["u"] == (e["tf"][0] * 4095, e["tf"][1] * 4094) and e["N"] == sum(e["u"]) < BC.TWO_POW_24
        for w in range(2):
            a, b = q["v"][w] * e["N"], e["u"][w] * q["N"]
            assert (a, b) == e["products"][w] and max(a, b) < 2 ** 48
            close += min(a, b) > 2 ** 44 and 0 < abs(a - b) < 2 ** 24
            entry_smaller += b < a
            query_smaller += a < b
            print("\nD products: word %d query's %d entry's %d difference %d" % (w, a, b, a - b), end="")
    print("\nwords with both products above 2^44 and closer than 2^24: %d; entry's smaller: %d; query's smaller: %d" % (close, entry_smaller, query_smaller))
    assert close >= 1 and entry_smaller >= 1 and query_smaller >= 1
    assert 4097 * 4095 == 2 ** 24 - 1 and 4096 * 4095 + 4096 * 1 == 2 ** 24 and 65535 * 4095 > 2 ** 24
    assert (2 ** 24 - 1) ** 2 < 2 ** 48 and float((2 ** 24 - 1) ** 2) == (2 ** 24 - 1) ** 2


# ---- the kernel's plain arithmetic on D and E ------------------------------------------------------------------------------
class Emu:
    """The host build of bow_weighted, bow_term, bow_score and bow_hit_before behind the same three calls; the ring and the gate
    are Python's. The bound on the norm is the kernel's BW_MAX_NORM, read from the same source text."""

    def __init__(self, lib, g):
        src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aria_slam_amd", "csrc", "bow_index.hip")).read()
        assert "constexpr int BW_MAX_NORM = 1 << 24;" in src and "N < (unsigned long long)BW_MAX_NORM && given >= 0 && (unsigned long long)given == N" in src
        self.L, self.g, self.db = lib, g, []
        self.idf = np.ascontiguousarray(g["idf"], np.uint16)

    def held(self, tf, norm):
        tf = np.ascontiguousarray(tf, np.uint16)
        N = self.L.emu_norm(tf.ctypes.data, self.idf.ctypes.data, len(self.idf))
        ok = N < (1 << 24) and norm >= 0 and int(norm) == N
        return (int(norm) if ok else 0), ok

    def add(self, ids, tf, norm):
        error = False
        for kid, t, n in zip(ids, tf, norm):
            n, ok = self.held(t, n)
            error |= not ok
            self.db = (self.db + [(int(kid), np.ascontiguousarray(t, np.uint16), n)])[-self.g["capacity"]:]
        return error

    def query(self, qids, tf, norm):
        hits, counts, error, K = [], [], False, self.g["top_k"]
        for qid, t, n in zip(qids, tf, norm):
            t = np.ascontiguousarray(t, np.uint16)
            n_q, ok = self.held(t, n)
            error |= not ok
            S, bits = np.zeros(len(self.db), np.int64), np.zeros(len(self.db), np.uint64)
            for e, (kid, tf_d, n_d) in enumerate(self.db):
                if n_q > 0 and n_d > 0 and int(qid) - kid >= self.g["mfb"]:
                    s, sc = C.c_longlong(0), C.c_double(0)
                    self.L.emu_score(t.ctypes.data, n_q, tf_d.ctypes.data, n_d, self.idf.ctypes.data, len(self.idf), C.byref(s), C.byref(sc))
                    S[e] = s.value
                    bits[e] = np.float64(sc.value).view(np.uint64) if s.value > 0 else 0
            out = np.zeros(K, np.int32)
            counts.append(self.L.emu_topk(bits.ctypes.data, len(self.db), K, out.ctypes.data))
            hits.append([(int(i), self.db[i][0], int(S[i]), int(bits[i])) if i >= 0 else BC.NONE for i in out])
        return hits, counts, error


@pytest.mark.parametrize("g", [g for g in INDEX if g["name"][0] in "DE"], ids=lambda g: g["name"])
def test_the_kernels_arithmetic_gives_the_answers_of_d_and_e(emu, g):   # noqa: F811
    assert differences(g, Emu(emu, g), size=lambda ix: len(ix.db), info=lambda ix, i: (ix.db[i][0], ix.db[i][2])) == []


# ---- wrong copies of the definition ----------------------------------------------------------------------------------------
WRONG = ["products kept in 32 bits", "factors masked to 20 bits", "the bound N <= 2^24", "ties to the higher index",
         "gate > instead of >=", "id difference in 32 bits", "the ring dropping the newest", "only the first 64 entries scored",
         "only the first 256 entries ranked", "words at or beyond 2048 dropped", "padding words read from the next row",
         "the second chunk answered with the first chunk's ids"]


@pytest.fixture(scope="module")
def old_table():
    """query_cases and the scene as groups of the same form, their answers from bow_ref (which the old tests hold to them)."""
    out = []
    for c in BC.query_cases():
        g = dict(name="query_cases " + c["name"], V=4, words=np.array(BC.QUERY_WORDS, np.uint8), idf=np.array(BC.QUERY_IDF, np.uint16),
                 capacity=c["capacity"], top_k=c["top_k"], mfb=c["mfb"], steps=[])
        if c["entries"]:
            tf = np.array([e[1] for e in c["entries"]], np.uint16)
            g["steps"].append(dict(op="add", tf=tf, norm=tf.sum(1).astype(np.int32), ids=[e[0] for e in c["entries"]], error=False))
        g["steps"].append(dict(op="state", size=c["size"], info=c["info"]))
        tf = np.array([q[1] for q in c["queries"]], np.uint16)
        g["steps"].append(dict(op="query", tf=tf, norm=tf.sum(1).astype(np.int32), qids=[q[0] for q in c["queries"]],
                               counts=[q[2] for q in c["queries"]], hits=[q[3] for q in c["queries"]], error=False))
        out.append(g)
    train, db, queries = BC.scene()
    words, idf, _ = R.train(train, BC.SCENE_WORDS, 10)
    g = dict(name="scene", V=BC.SCENE_WORDS, words=words, idf=idf, capacity=64, top_k=4, mfb=10, steps=[])
    bags = [R.transform(v, words, idf) for v in db]
    g["steps"].append(dict(op="add", tf=np.stack([b[0] for b in bags]), norm=[b[1] for b in bags], ids=list(range(len(bags))), error=False))
    qb = [R.transform(v, words, idf) for v in queries]
    ref = Ref(g)
    ref.add(*[g["steps"][0][k] for k in ("ids", "tf", "norm")])
    hits, counts, _ = ref.query([1000 + p for p in range(len(qb))], [b[0] for b in qb], [b[1] for b in qb])
    g["steps"].append(dict(op="query", tf=np.stack([b[0] for b in qb]), norm=[b[1] for b in qb], qids=[1000 + p for p in range(len(qb))],
                           counts=counts, hits=hits, error=False))
    out.append(g)
    return out


def test_the_double_loop_is_the_definition_on_the_old_table(old_table):
    for g in old_table:
        assert _copy_differences(g) == [], g["name"]


def test_wrong_copies_of_the_definition(old_table):
    """Every mistake changes an answer of at least one edge group; which of them the old table notices is printed and, for
    the record, asserted as it stands."""
    sees_old = {}
    print()
    for wrong in WRONG:
        old = [g["name"] for g in old_table if _copy_differences(g, wrong)]
        new = [g["name"] for g in INDEX if _copy_differences(g, wrong)]
        sees_old[wrong] = bool(old)
        print("%-55s old table: %-28s edge groups: %s" % (wrong, ", ".join(old) or "blind", ", ".join(new)))
        assert new, wrong
    # the old table's V = 4 has a row stride of 8, so it does meet padding words, in the first trip of the row loop only
    assert [w for w in WRONG if sees_old[w]] == ["ties to the higher index", "gate > instead of >=", "the ring dropping the newest",
                                                 "padding words read from the next row"]


# ---- group F ---------------------------------------------------------------------------------------------------------------
def test_transform_at_size_gives_the_written_rows():
    g = BY_NAME["F transform V=4096"]
    assert len(g["frames"]) == 300 and g["error"] and all(f >= 256 for f in BC.F_REFUSED)
    for f in g["sample"] + list(range(250, 262)):
        valid = 0 <= g["counts"][f] <= g["rows"]
        tf, N = R.transform(g["frames"][f][:g["counts"][f]] if valid else g["frames"][f][:0], g["words"], g["idf"])
        assert tf.tobytes() == g["tf"][f].tobytes() and N == g["norm"][f], f
    assert g["tf"][BC.F_ONE_WORD].tolist() == [0] * 4095 + [4096] and g["norm"][BC.F_ONE_WORD] == 4096 * 4095 < BC.TWO_POW_24
    # every other frame: its descriptors ARE words, so the row is the count of each word named
    for f in range(300):
        want = np.zeros(4096, np.int64)
        if f not in BC.F_REFUSED:
            np.add.at(want, [int(d[0]) | int(d[1]) << 8 for d in g["frames"][f]], 1)
        assert want.tolist() == g["tf"][f].tolist() and int((want * g["idf"]).sum()) == g["norm"][f]


def test_census_of_the_training_sets():
    """With the restatement alone: the V = 4096 set has words without members, with exactly one, with more than 256, a majority
    tie, and a word that changes in an iteration after the first; the V = 33 set has empty frames from index 256 on."""
    g = BY_NAME["F train V=4096"]
    D = np.concatenate(g["frames"])
    n, V = len(D), g["V"]
    assert len(g["frames"]) == 30 and all(len(f) == 400 for f in g["frames"])
    words = D[[(j * n) // V for j in range(V)]].copy()
    rows = []
    for it in range(g["iters"]):
        idx = R.quantise(D, words)
        members = np.bincount(idx, minlength=V)
        ones = np.zeros((V, 256), np.int64)
        np.add.at(ones, idx, R.bits_of(D).astype(np.int64))
        new = R.majority(D, idx, words)
        rows.append(dict(none=int((members == 0).sum()), one=int((members == 1).sum()), over_256=int((members > 256).sum()),
                         most=int(members.max()), ties=int(((2 * ones == members[:, None]) & (members[:, None] > 0)).any(1).sum()),
                         changed=int((new != words).any(1).sum())))
        words = new
    print("\nF train V=4096, per iteration:", rows)
    assert rows[0]["none"] > 0 and rows[0]["one"] > 0 and rows[0]["over_256"] > 0 and rows[0]["ties"] > 0 and rows[1]["changed"] > 0
    got = R.train(g["frames"], V, g["iters"])
    assert got[0].tobytes() == words.tobytes() and got[2] == 3 and len(set(got[1].tolist())) > 4
    s = BY_NAME["F train V=33"]
    lens = [len(f) for f in s["frames"]]
    assert len(lens) == 300 and set(lens) == {0, 1, 2, 3} and all(lens[f] == 0 for f in range(256, 300, 2)) and sum(lens[256:]) > 0
    w33, idf33, run33 = R.train(s["frames"], 33, s["iters"])
    print("F train V=33: %d descriptors, %d iterations, weights %s" % (sum(lens), run33, sorted(set(idf33.tolist()))))
    assert sum(lens) >= 33 and run33 >= 2
