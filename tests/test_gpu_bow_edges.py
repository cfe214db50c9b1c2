"""The edge groups of the place-recognition stage (tests/bow_cases.py, edge_groups()) on the MI355X through HipBowIndex: every
tile of k_bow_score and every wave and trip of k_bow_topk (group A), the ring at every head and the chunks of an add (B), the
chunks of a query call, the gate and 64-bit ids (C), the bound on the norm and 48-bit products decided below bit 24 (D), every row
stride and guard of the score kernel's row loop (E), transform and training at V = 4096 and beyond 256 frames (F). Every output
lies between guards of 0x5A and is compared as bytes with the answers written down from the constructions (training: with the
restatement); a sample of every batch is asked again one query, one frame at a time and gives the same bytes; a deferred error is
reported once. tests/test_bow_edges_host.py holds the restatement to the same answers and counts what the groups reach."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_cases as BC   # noqa: E402
from test_bow_edges_host import GROUPS, differences   # noqa: E402
from test_gpu_bow import GUARD, INVALID, _body, _dev, _guarded, _transform, torch_cuda, work   # noqa: E402,F401


class Device:
    """One HipBowIndex behind the three calls a group's steps are run with (differences() of the host test)."""

    def __init__(self, aria, torch, work, g):   # noqa: F811
        self.torch, self.work, self.g = torch, work, g
        self.ix = aria.HipBowIndex(rows=g["rows"], capacity=g["capacity"], top_k=g["top_k"], min_frames_between=g["mfb"],
                                   stream=work.cuda_stream)
        self.ix.set_vocabulary(g["words"], g["idf"])
        assert self.ix.words == g["V"] and self.ix.size() == 0

    def _reported_once(self):
        status = self.ix.status()
        assert status in (0, INVALID) and self.ix.status() == 0
        return status == INVALID

    def add(self, ids, tf, norm):
        self.ix.add_batch_device(_dev(self.torch, self.work, np.asarray(tf, np.uint16)), _dev(self.torch, self.work, np.asarray(norm, np.int32)), ids)
        return self._reported_once()

    def _ask(self, qids, tf, norm):
        from aria_slam_amd._lib import BOW_HIT_DTYPE
        n, K = len(qids), self.ix.top_k
        d_hits, d_counts = _guarded(self.torch, self.work, n * K * 32), _guarded(self.torch, self.work, n * 4)
        self.ix.query_batch_device(_dev(self.torch, self.work, np.asarray(tf, np.uint16)), _dev(self.torch, self.work, np.asarray(norm, np.int32)),
                                   qids, d_hits[GUARD:], d_counts[GUARD:])
        error = self._reported_once()
        return _body(d_hits, BOW_HIT_DTYPE).reshape(n, K), _body(d_counts, np.int32), error

    def query(self, qids, tf, norm):
        hits, counts, error = self._ask(qids, tf, norm)
        step = next(s for s in self.g["steps"] if s["op"] == "query" and s["tf"] is tf)
        idf = [int(x) for x in self.g["idf"]]
        for j in step["sample"]:                     # the same query alone: the same bytes, and its own error alone
            h1, c1, e1 = self._ask(qids[j:j + 1], tf[j:j + 1], norm[j:j + 1])
            refused = not 0 <= int(norm[j]) == sum(int(t) * w for t, w in zip(tf[j], idf)) < BC.TWO_POW_24
            assert h1[0].tobytes() == hits[j].tobytes() and c1[0] == counts[j] and e1 == refused, (self.g["name"], j)
        return list(hits), counts.tolist(), error


@pytest.mark.parametrize("g", [g for g in GROUPS if g["kind"] == "index"], ids=lambda g: g["name"])
def test_index_group(aria, torch_cuda, work, g):   # noqa: F811
    dev = Device(aria, torch_cuda, work, g)
    try:
        assert differences(g, dev, size=lambda d: d.ix.size(), info=lambda d, i: d.ix.info(i)) == []
        with pytest.raises(aria.AriaError):
            dev.ix.info(dev.ix.size())
    finally:
        dev.ix.close()


def test_transform_at_size(aria, torch_cuda, work):   # noqa: F811
    """300 frames in one call at V = 4096: the second block of k_bow_counts with a refused -1 and rows + 1 in it, 4096
    descriptors on one word (4096 LDS atomics on one counter, tf = 4096, the largest norm a frame can have), one on every word."""
    g = next(g for g in GROUPS if g["kind"] == "transform")
    ix = aria.HipBowIndex(rows=g["rows"], capacity=4, stream=work.cuda_stream)
    try:
        ix.set_vocabulary(g["words"], g["idf"])
        tf, norm, status = _transform(torch_cuda, work, ix, g["frames"], g["counts"], g["stride"])
        assert tf.tobytes() == g["tf"].tobytes() and norm.tobytes() == np.array(g["norm"], np.int32).tobytes()
        assert status == INVALID and ix.status() == 0
        for f in g["sample"]:
            tf1, norm1, status1 = _transform(torch_cuda, work, ix, [g["frames"][f]], [g["counts"][f]], g["stride"])
            assert tf1[0].tobytes() == g["tf"][f].tobytes() and norm1[0] == g["norm"][f], f
            assert status1 == (INVALID if f in BC.F_REFUSED else 0) and ix.status() == 0
    finally:
        ix.close()


@pytest.mark.parametrize("g", [g for g in GROUPS if g["kind"] == "train"], ids=lambda g: g["name"])
def test_training_at_size(aria, torch_cuda, work, g):   # noqa: F811
    """Words, weights and iterations run, bit for bit with the restatement, and the same bytes when trained again."""
    from aria_slam_amd import bow_ref as R
    want = R.train(g["frames"], g["V"], g["iters"])
    ix = aria.HipBowIndex(words=g["V"], rows=512, capacity=4, train_iters=g["iters"], stream=work.cuda_stream)
    try:
        for _ in range(2):
            run = ix.train(g["frames"])
            words, idf = ix.vocabulary()
            assert run == want[2] and ix.words == g["V"] and ix.status() == 0
            assert words.tobytes() == want[0].tobytes() and idf.tobytes() == want[1].tobytes()
    finally:
        ix.close()
