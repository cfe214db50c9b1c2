"""Place recognition on the MI355X (aria_bow_*, kernels in aria_slam_amd/csrc/bow_index.hip) against its definition, the NumPy
restatement aria_slam_amd/bow_ref.py, bit for bit: words, weights, iterations run, bags, norms, hits with the numerator S and the
bit pattern of the score, counts and deferred errors; on the case table (tests/bow_cases.py) equal to the answers written down
from the construction as well.

This file holds the rules at small sizes: at most 40 entries, 40 bags in a call and top_k 4, queries at V = 4, 256 and 4096, the
ring wrapping at capacity 4. More than one tile of k_bow_score, more than one wave or trip of k_bow_topk, a second chunk of an add or
a query call, the other row strides, the bound on the norm and training and transform at size are tests/test_gpu_bow_edges.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_cases as BC   # noqa: E402

GUARD = 256                                   # bytes of 0x5A before and after every output
INVALID = -1                                  # ARIA_E_INVALID


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


def _dev(torch, work, a):
    with torch.cuda.stream(work):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    work.synchronize()
    return t


def _guarded(torch, work, nbytes):
    with torch.cuda.stream(work):
        t = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _body(t, dtype):
    raw = t.cpu().numpy()
    assert (raw[:GUARD] == 0x5A).all() and (raw[-GUARD:] == 0x5A).all(), "a guard byte around an output was written"
    return raw[GUARD:-GUARD].copy().view(dtype)


def _block(frames, stride):
    out = np.zeros((len(frames), stride, 32), np.uint8)
    for k, f in enumerate(frames):
        out[k, :len(f)] = f
    return out


def _transform(torch, work, ix, frames, counts, stride):
    """aria_bow_transform_batch_device on host arrays -> (tf [F, V] uint16, norm [F] int32, status)."""
    F, V = len(frames), ix.words
    d_desc, d_counts = _dev(torch, work, _block(frames, stride)), _dev(torch, work, np.asarray(counts, np.int32))
    d_tf, d_norm = _guarded(torch, work, F * V * 2), _guarded(torch, work, F * 4)
    ix.transform_batch_device(d_desc, d_counts, F, stride, d_tf[GUARD:], d_norm[GUARD:])
    status = ix.status()
    return _body(d_tf, np.uint16).reshape(F, V), _body(d_norm, np.int32), status


def _query(torch, work, ix, tf, norm, qids):
    """aria_bow_query_batch_device on host arrays -> (hits [n, K], counts [n])."""
    from aria_slam_amd._lib import BOW_HIT_DTYPE
    n, K = len(qids), ix.top_k
    d_tf, d_norm = _dev(torch, work, np.asarray(tf, np.uint16)), _dev(torch, work, np.asarray(norm, np.int32))
    d_hits, d_counts = _guarded(torch, work, n * K * 32), _guarded(torch, work, n * 4)
    ix.query_batch_device(d_tf, d_norm, qids, d_hits[GUARD:], d_counts[GUARD:])
    assert ix.status() == 0
    return _body(d_hits, BOW_HIT_DTYPE).reshape(n, K), _body(d_counts, np.int32)


@pytest.mark.parametrize("c", BC.train_cases(), ids=lambda c: c["name"])
def test_train_cases(aria, torch_cuda, work, c):
    from aria_slam_amd import bow_ref as R
    if c["V"] < 1 or c["V"] > 4096:
        with pytest.raises(aria.AriaError):
            aria.HipBowIndex(words=c["V"], stream=work.cuda_stream)
        return
    ix = aria.HipBowIndex(words=c["V"], rows=512, capacity=4, train_iters=c["iters"], stream=work.cuda_stream)
    try:
        if c.get("refused"):
            with pytest.raises(aria.AriaError):
                ix.train(c["frames"])
            assert ix.words == 0
            return
        run = ix.train(c["frames"])
        words, idf = ix.vocabulary()
        want = R.train(c["frames"], c["V"], c["iters"])
        assert words.tobytes() == want[0].tobytes() == np.array(c["words"], np.uint8).tobytes()
        assert idf.tolist() == want[1].tolist() == list(c["idf"])
        assert run == want[2] == c["run"] and ix.words == c["V"] and ix.status() == 0
    finally:
        ix.close()


@pytest.mark.parametrize("c", BC.transform_cases(), ids=lambda c: c["name"])
def test_transform_cases(aria, torch_cuda, work, c):
    ix = aria.HipBowIndex(rows=c["rows"], capacity=4, stream=work.cuda_stream)
    try:
        ix.set_vocabulary(c["words"], c["idf"])
        tf, norm, status = _transform(torch_cuda, work, ix, c["frames"], c["counts"], c["stride"])
        assert tf.tolist() == c["tf"] and norm.tolist() == c["norm"]
        assert status == (INVALID if c["error"] else 0) and ix.status() == 0          # reported once
        # the same frames one at a time: the shared train set of the batched kNN call changes nothing
        for f, (cnt, desc) in enumerate(zip(c["counts"], c["frames"])):
            tf1, norm1, status1 = _transform(torch_cuda, work, ix, [desc], [cnt], c["stride"])
            assert tf1[0].tolist() == c["tf"][f] and norm1[0] == c["norm"][f]
            assert status1 == (0 if 0 <= cnt <= c["rows"] else INVALID)
    finally:
        ix.close()


@pytest.mark.parametrize("c", BC.query_cases(), ids=lambda c: c["name"])
def test_query_cases(aria, torch_cuda, work, c):
    torch = torch_cuda
    ix = aria.HipBowIndex(rows=16, capacity=c["capacity"], top_k=c["top_k"], min_frames_between=c["mfb"], stream=work.cuda_stream)
    try:
        ix.set_vocabulary(BC.QUERY_WORDS, BC.QUERY_IDF)
        if c["entries"]:
            tf = np.array([e[1] for e in c["entries"]], np.uint16)
            ix.add_batch_device(_dev(torch, work, tf), _dev(torch, work, tf.sum(1).astype(np.int32)), [e[0] for e in c["entries"]])
        assert ix.status() == 0 and ix.size() == c["size"]
        for index, kid, norm in c["info"]:
            assert ix.info(index) == (kid, norm)
        with pytest.raises(aria.AriaError):
            ix.info(c["size"])
        qtf = np.array([q[1] for q in c["queries"]], np.uint16)
        qn, qids = qtf.sum(1).astype(np.int32), [q[0] for q in c["queries"]]
        hits, counts = _query(torch, work, ix, qtf, qn, qids)
        for k, (qid, _, count, want) in enumerate(c["queries"]):
            assert counts[k] == count and hits[k].tobytes() == BC.expected_hits(want).tobytes(), (c["name"], k, hits[k])
            one_h, one_c = _query(torch, work, ix, qtf[k:k + 1], qn[k:k + 1], qids[k:k + 1])            # a batch of one
            assert one_c[0] == count and one_h[0].tobytes() == hits[k].tobytes()
    finally:
        ix.close()


def test_a_norm_that_is_not_the_bags_is_refused_alone(aria, torch_cuda, work):
    torch = torch_cuda
    ix = aria.HipBowIndex(rows=16, capacity=4, top_k=2, min_frames_between=0, stream=work.cuda_stream)
    try:
        ix.set_vocabulary(BC.QUERY_WORDS, BC.QUERY_IDF)
        tf = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], np.uint16)
        ix.add_batch_device(_dev(torch, work, tf), _dev(torch, work, np.array([1, 2, 1], np.int32)), [0, 1, 2])
        assert ix.status() == INVALID and ix.status() == 0
        assert [ix.info(i) for i in range(3)] == [(0, 1), (1, 0), (2, 1)]
        hits, counts = _query(torch, work, ix, tf[:1], [1], [9])
        assert counts[0] == 2 and hits[0]["index"].tolist() == [0, 2]
        # the same for a query: it alone is an empty query, its neighbours are answered
        from aria_slam_amd._lib import BOW_HIT_DTYPE
        d_hits, d_counts = _guarded(torch, work, 3 * 2 * 32), _guarded(torch, work, 3 * 4)
        ix.query_batch_device(_dev(torch, work, tf), _dev(torch, work, np.array([1, 7, 1], np.int32)), [9, 9, 9], d_hits[GUARD:], d_counts[GUARD:])
        assert ix.status() == INVALID and ix.status() == 0
        got = _body(d_hits, BOW_HIT_DTYPE).reshape(3, 2)
        assert _body(d_counts, np.int32).tolist() == [2, 0, 2] and got[1]["index"].tolist() == [-1, -1]
        assert got[0].tobytes() == got[2].tobytes() == hits[0].tobytes()
    finally:
        ix.close()


@pytest.fixture(scope="module")
def scene():
    """The generated scene and its restatement, computed once."""
    from aria_slam_amd import bow_ref as R
    train, db, queries = BC.scene()
    words, idf, run = R.train(train, BC.SCENE_WORDS, 10)
    ref = R.BowIndexRef(words, idf, capacity=64, top_k=4, min_frames_between=10)
    bags = [ref.transform(v) for v in db]
    for p, (tf, n) in enumerate(bags):
        ref.add_bag(p, tf, n)
    qbags = [ref.transform(v) for v in queries]
    want = [ref.query_bag(1000 + p, tf, n) for p, (tf, n) in enumerate(qbags)]
    return dict(train=train, db=db, queries=queries, words=words, idf=idf, run=run, bags=bags, qbags=qbags, want=want)


def _scene_index(aria, work, **kw):
    return aria.HipBowIndex(words=BC.SCENE_WORDS, rows=256, capacity=64, top_k=4, min_frames_between=10, stream=work.cuda_stream, **kw)


def test_scene_on_the_device_is_the_restatement(aria, torch_cuda, work, scene):
    """Training, bags and hits of the 40-place scene, bit for bit; so 40 of 40 first. Training twice gives the same bytes; a
    batch of queries equals the same queries one at a time; the host forms equal the batch forms."""
    torch = torch_cuda
    ix = _scene_index(aria, work)
    try:
        run = ix.train(scene["train"])
        words, idf = ix.vocabulary()
        assert run == scene["run"] and words.tobytes() == scene["words"].tobytes() and idf.tobytes() == scene["idf"].tobytes()
        assert ix.train(scene["train"]) == run
        again = ix.vocabulary()
        assert again[0].tobytes() == words.tobytes() and again[1].tobytes() == idf.tobytes()

        tf, norm, status = _transform(torch, work, ix, scene["db"], [len(v) for v in scene["db"]], BC.SCENE_VIEW)
        assert status == 0
        assert tf.tobytes() == np.stack([b[0] for b in scene["bags"]]).tobytes() and norm.tolist() == [b[1] for b in scene["bags"]]
        ix.add_batch_device(_dev(torch, work, tf), _dev(torch, work, norm), list(range(len(tf))))
        assert ix.size() == BC.SCENE_PLACES

        qtf, qn, _ = _transform(torch, work, ix, scene["queries"], [len(v) for v in scene["queries"]], BC.SCENE_VIEW)
        assert qtf.tobytes() == np.stack([b[0] for b in scene["qbags"]]).tobytes()
        qids = [1000 + p for p in range(BC.SCENE_PLACES)]
        hits, counts = _query(torch, work, ix, qtf, qn, qids)
        for p, (want, count) in enumerate(scene["want"]):
            assert counts[p] == count and hits[p].tobytes() == want.tobytes(), p
        assert (hits[:, 0]["index"] == np.arange(BC.SCENE_PLACES)).all()
        for p in (0, 17, 39):
            h1, c1 = _query(torch, work, ix, qtf[p:p + 1], qn[p:p + 1], qids[p:p + 1])
            assert c1[0] == counts[p] and h1[0].tobytes() == hits[p].tobytes()
            h2, c2 = ix.query(qids[p], scene["queries"][p])
            assert c2 == counts[p] and h2.tobytes() == hits[p].tobytes()
            h3, c3 = ix.query_device(qids[p], _dev(torch, work, scene["queries"][p]), len(scene["queries"][p]))
            assert c3 == counts[p] and h3.tobytes() == hits[p].tobytes()
    finally:
        ix.close()


def test_save_load_and_a_truncated_file(aria, torch_cuda, work, scene, tmp_path):
    from aria_slam_amd import bow_ref as R
    a, b = _scene_index(aria, work), _scene_index(aria, work)
    try:
        with pytest.raises(aria.AriaError):
            a.save(str(tmp_path / "none.bow"))                                 # no vocabulary yet
        with pytest.raises(aria.AriaError):
            a.add(0, scene["db"][0])
        a.set_vocabulary(scene["words"], scene["idf"])
        path = str(tmp_path / "scene.bow")
        a.save(path)
        blob = open(path, "rb").read()
        assert blob == R.vocabulary_bytes(scene["words"], scene["idf"])
        b.load(path)
        assert b.vocabulary()[0].tobytes() == scene["words"].tobytes() and b.vocabulary()[1].tobytes() == scene["idf"].tobytes()
        for ix in (a, b):                                                      # the host add: one frame at a time
            for p, v in enumerate(scene["db"]):
                ix.add(p, v)
        for p in (3, 21):
            ha, ca = a.query(1000 + p, scene["queries"][p])
            hb, cb = b.query(1000 + p, scene["queries"][p])
            assert ca == cb == scene["want"][p][1] and ha.tobytes() == hb.tobytes() == scene["want"][p][0].tobytes()
        for name, bad in (("short", blob[:-1]), ("head", blob[:10]), ("long", blob + b"\0"), ("magic", b"X" + blob[1:]),
                          ("version", blob[:8] + b"\x02" + blob[9:]), ("zero", blob[:12] + bytes(4) + blob[16:])):
            p = str(tmp_path / (name + ".bow"))
            open(p, "wb").write(bad)
            with pytest.raises(aria.AriaError):
                b.load(p)
        with pytest.raises(aria.AriaError):
            b.load(str(tmp_path / "absent.bow"))
        assert b.words == BC.SCENE_WORDS and b.size() == BC.SCENE_PLACES       # a refused file changes nothing
    finally:
        a.close()
        b.close()


def test_drop_at_capacity_through_the_host_add(aria, torch_cuda, work):
    ix = aria.HipBowIndex(rows=16, capacity=4, top_k=4, min_frames_between=0, stream=work.cuda_stream)
    try:
        ix.set_vocabulary(BC.QUERY_WORDS, BC.QUERY_IDF)
        W = np.array(BC.QUERY_WORDS, np.uint8)
        for kid, words in enumerate(([0], [1], [2], [3], [0, 1], [])):         # ids 0 and 1 are dropped, id 5 is empty
            ix.add(kid, W[words])
        assert ix.size() == 4 and [ix.info(i) for i in range(4)] == [(2, 1), (3, 1), (4, 2), (5, 0)]
        hits, count = ix.query(100, W[[1]])
        assert count == 1 and hits[0]["index"] == 2 and hits[0]["id"] == 4 and hits[0]["S"] == 1 and hits[0]["score"] == 0.5
        assert hits[1:]["index"].tolist() == [-1, -1, -1]
        with pytest.raises(aria.AriaError):
            ix.add(6, np.zeros((17, 32), np.uint8))                            # more than rows
    finally:
        ix.close()


def test_full_size_vocabulary_once(aria, torch_cuda, work):
    """V = 4096 and a pair of 2000-descriptor frames: the full-size LDS layout of the histogram and of the score kernel."""
    from aria_slam_amd import bow_ref as R
    rng = np.random.default_rng(11)
    words = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    idf = rng.integers(0, 4096, 4096).astype(np.uint16)
    frames = [words[rng.integers(0, 4096, 2000)].copy() for _ in range(2)]
    for f in frames:
        f[:, 5] ^= rng.integers(0, 4, 2000).astype(np.uint8)                   # at most two bits from a word
    ix = aria.HipBowIndex(rows=2000, capacity=2, top_k=2, min_frames_between=0, stream=work.cuda_stream)
    try:
        ix.set_vocabulary(words, idf)
        tf, norm, status = _transform(torch_cuda, work, ix, frames, [2000, 2000], 2000)
        want = [R.transform(f, words, idf) for f in frames]
        assert status == 0 and tf.tobytes() == np.stack([w[0] for w in want]).tobytes() and norm.tolist() == [w[1] for w in want]
        ix.add_batch_device(_dev(torch_cuda, work, tf), _dev(torch_cuda, work, norm), [0, 1])
        hits, counts = _query(torch_cuda, work, ix, tf, norm, [5, 5])
        ref = R.BowIndexRef(words, idf, capacity=2, top_k=2, min_frames_between=0)
        for kid, (t, n) in enumerate(want):
            ref.add_bag(kid, t, n)
        for k, (t, n) in enumerate(want):
            h, c = ref.query_bag(5, t, n)
            assert counts[k] == c and hits[k].tobytes() == h.tobytes()
        assert hits[0, 0]["index"] == 0 and hits[0, 0]["score"] == 1.0 and hits[1, 0]["index"] == 1
    finally:
        ix.close()


def test_handle_lifecycle_on_a_borrowed_and_an_owned_stream(aria, torch_cuda, work, scene):
    """The host forms on a handle that owns its stream and on one that borrows the test's; a handle destroyed with work in
    flight; the borrowed stream outlives the handles."""
    torch = torch_cuda
    for stream in (None, work.cuda_stream):
        ix = aria.HipBowIndex(words=BC.SCENE_WORDS, rows=256, capacity=64, top_k=4, min_frames_between=10, stream=stream)
        assert (ix.stream == work.cuda_stream) == (stream is not None) and ix.stream
        ix.set_vocabulary(scene["words"], scene["idf"])
        for p in range(6):
            ix.add(p, scene["db"][p])
        hits, count = ix.query(1002, scene["queries"][2])
        assert count >= 1 and hits[0]["index"] == 2
        # destroy with work in flight: a batch transform and a query enqueued, nothing read back
        d_desc = _dev(torch, work, _block(scene["db"], BC.SCENE_VIEW))
        d_counts = _dev(torch, work, np.full(BC.SCENE_PLACES, BC.SCENE_VIEW, np.int32))
        d_tf, d_norm = _guarded(torch, work, BC.SCENE_PLACES * BC.SCENE_WORDS * 2), _guarded(torch, work, BC.SCENE_PLACES * 4)
        d_hits, d_cnt = _guarded(torch, work, BC.SCENE_PLACES * 4 * 32), _guarded(torch, work, BC.SCENE_PLACES * 4)
        ix.transform_batch_device(d_desc, d_counts, BC.SCENE_PLACES, BC.SCENE_VIEW, d_tf[GUARD:], d_norm[GUARD:])
        ix.query_batch_device(d_tf[GUARD:], d_norm[GUARD:], list(range(1000, 1000 + BC.SCENE_PLACES)), d_hits[GUARD:], d_cnt[GUARD:])
        ix.close()
        ix.close()                                                             # idempotent
        assert _body(d_norm, np.int32).tolist() == [b[1] for b in scene["bags"]]                         # it was drained, not dropped
    with torch.cuda.stream(work):
        t = torch.ones(16, device="cuda:0").sum()
    work.synchronize()
    assert float(t) == 16.0


def test_find_candidates_bow_is_a_subset_of_the_full_scan(aria, torch_cuda, work, scene):
    """KeyframeDB.find_candidates_bow on the scene: the index names four slots, the exact scan runs on those alone, and what it
    returns is what find_candidates returns for the same slots, the right place first."""
    from aria_slam_amd import loopdb
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rows = 256
    db = loopdb.KeyframeDB(k_cap=64, rows=rows, device=dev)
    m = aria.HipMatcher(device=0, max_query=rows, max_train=rows)
    ix = _scene_index(aria, work)
    try:
        ix.set_vocabulary(scene["words"], scene["idf"])
        for p, v in enumerate(scene["db"]):
            d = torch.from_numpy(v).to(dev)
            torch.cuda.synchronize()
            db.add(p, d, len(v))
            ix.add_device(p, d, len(v))
        torch.cuda.synchronize()
        assert ix.size() == db.n == BC.SCENE_PLACES
        for p in (0, 13, 39):
            q = scene["queries"][p]
            dq = torch.from_numpy(q).to(dev)
            torch.cuda.synchronize()
            full = db.find_candidates(m, dq, len(q), 1000 + p, 10)
            got = db.find_candidates_bow(m, ix, dq, len(q), 1000 + p, 10)
            named = set(int(i) for i in scene["want"][p][0]["index"] if i >= 0)
            assert got and got[0][0] == p and set(i for i, _ in got) <= named
            assert [c for c in full if c[0] in named] == got
    finally:
        ix.close()
        m.close()
