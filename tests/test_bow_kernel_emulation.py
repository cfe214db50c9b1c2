"""The kernel source of aria_slam_amd/csrc/bow_index.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/bow_ref.py) on the case table tests/test_gpu_bow.py runs on the device.

The plain arithmetic between the file's two marker comments -- the majority rule, the integer logarithm and the weight, a word's
weighted count (the norm), the per-word min of 64-bit products, the one division of the score, and the comparison that orders
hits -- is pasted between tests/cpp/bow_kernel_emu_head.inc and bow_kernel_emu_tail.inc and compiled with the clang++ that hipcc
drives. The tail restates the kernels' loops around those functions.

What this cannot check: the LDS histogram and its atomics, the member lists (scan, scatter and their atomics), the shuffles that
assemble a word and reduce sums and hits, the ring's slots, and the kNN call that quantises. That is tests/test_gpu_bow.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_cases as BC   # noqa: E402
from aria_slam_amd import bow_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "bow_index.hip")).read()
    plain = src[src.index("// ---- the plain arithmetic of the stage"):src.index("// ---- end of the plain arithmetic ----")]
    for fn in ("bow_majority_bit", "bow_ilog2_q8", "bow_idf", "bow_weighted", "bow_term", "bow_score", "bow_hit_before"):
        assert fn in plain, fn
    for word in ("__shared__", "__syncthreads", "__shfl", "__ballot", "atomic", "asm", "log2f", "std::log", "<cmath>"):
        assert word not in plain, "plain HIP C++: no LDS, no barrier, no cross-lane operation, no libm (%s)" % word
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("bow_kernel_emu_head.inc", "bow_kernel_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "bow_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "bow_emu.cpp"), os.path.join(out_dir, "libbow_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + plain + parts[1])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, cpp])
    L = C.CDLL(so)
    p, i, u = C.c_void_p, C.c_int, C.c_uint
    L.emu_ilog2_q8.argtypes, L.emu_ilog2_q8.restype = [u, u], u
    L.emu_idf.argtypes, L.emu_idf.restype = [u, u], u
    L.emu_majority.argtypes, L.emu_majority.restype = [p, u, p], None
    L.emu_norm.argtypes, L.emu_norm.restype = [p, p, i], C.c_longlong
    L.emu_score.argtypes, L.emu_score.restype = [p, i, p, i, p, i, p, p], None
    L.emu_topk.argtypes = [p, i, i, p]
    return L


def test_integer_logarithm_and_weight(emu):
    for F, n_w, want in BC.ILOG:
        assert emu.emu_ilog2_q8(F, n_w) == want == R.ilog2_q8(F, n_w)
    for F, n_w, want in BC.IDF:
        assert emu.emu_idf(F, n_w) == want == R.idf_weight(F, n_w)
    rng = np.random.default_rng(2)
    for _ in range(4000):
        F = int(rng.integers(1, 65536))
        n_w = int(rng.integers(1, F + 1))
        assert emu.emu_ilog2_q8(F, n_w) == R.ilog2_q8(F, n_w), (F, n_w)
    for F in (1, 2, 3, 255, 256, 65535):
        for n_w in range(0, min(F, 300) + 1):
            assert emu.emu_idf(F, n_w) == R.idf_weight(F, n_w), (F, n_w)


def _majority(emu, desc, idx, words):
    out = np.array(words, np.uint8).copy()
    bits = R.bits_of(desc).astype(np.uint32)
    for w in range(len(out)):
        mine = bits[np.asarray(idx) == w]
        ones = np.ascontiguousarray(mine.sum(0), np.uint32) if len(mine) else np.zeros(256, np.uint32)
        emu.emu_majority(ones.ctypes.data, len(mine), out[w].ctypes.data)
    return out


@pytest.mark.parametrize("c", [c for c in BC.train_cases() if not c.get("refused")], ids=lambda c: c["name"])
def test_majority_rule_on_the_train_cases(emu, c):
    """The restatement's training loop with the kernel's majority rule and weight in place of its own."""
    D = np.concatenate(c["frames"])
    n, V = len(D), c["V"]
    words = D[[(j * n) // V for j in range(V)]].copy()
    run = 0
    while run < c["iters"]:
        idx = R.quantise(D, words)
        new = _majority(emu, D, idx, words)
        assert new.tobytes() == R.majority(D, idx, words).tobytes()
        run += 1
        changed = new.tobytes() != words.tobytes()
        words = new
        if not changed:
            break
    assert words.tobytes() == np.array(c["words"], np.uint8).tobytes() and run == c["run"]
    n_w = [sum(1 for f in c["frames"] if len(f) and (R.quantise(f, words) == w).any()) for w in range(V)]
    assert [emu.emu_idf(len(c["frames"]), k) for k in n_w] == list(c["idf"])


def test_majority_rule_random(emu):
    rng = np.random.default_rng(4)
    D = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    words = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    idx = rng.integers(0, 6, 300)                                           # word 6 has no members
    assert _majority(emu, D, idx, words).tobytes() == R.majority(D, idx, words).tobytes()


def _score(emu, tq, nq, td, nd, idf):
    tq, td, idf = (np.ascontiguousarray(a, np.uint16) for a in (tq, td, idf))
    S, sc = C.c_longlong(0), C.c_double(0)
    emu.emu_score(tq.ctypes.data, nq, td.ctypes.data, nd, idf.ctypes.data, len(idf), C.byref(S), C.byref(sc))
    return S.value, sc.value


@pytest.mark.parametrize("c", BC.query_cases(), ids=lambda c: c["name"])
def test_score_and_order_on_the_query_cases(emu, c):
    """The database as a list, the gate in Python, the kernel's numerator, division and ordering."""
    entries = c["entries"][-c["capacity"]:]
    idf = np.array(BC.QUERY_IDF, np.uint16)
    for qid, tf, count, want in c["queries"]:
        nq = sum(tf)
        assert emu.emu_norm(np.array(tf, np.uint16).ctypes.data, idf.ctypes.data, 4) == nq
        S = np.zeros(max(len(entries), 1), np.int64)
        bits = np.zeros(max(len(entries), 1), np.uint64)
        for e, (kid, tfd) in enumerate(entries):
            nd = sum(tfd)
            if nq > 0 and nd > 0 and qid - kid >= c["mfb"]:
                S[e], sc = _score(emu, tf, nq, tfd, nd, idf)
                bits[e] = np.float64(sc).view(np.uint64) if S[e] > 0 else 0
        out = np.zeros(c["top_k"], np.int32)
        assert emu.emu_topk(bits.ctypes.data, len(entries), c["top_k"], out.ctypes.data) == count
        got = [(int(i), entries[i][0], int(S[i]), int(bits[i])) if i >= 0 else BC.NONE for i in out]
        assert got == list(want), (c["name"], qid, tf)


def test_score_bit_budget_and_random_bags(emu):
    idf = np.array([4095, 4095], np.uint16)
    tf = np.array([4096, 0], np.uint16)
    N = emu.emu_norm(tf.ctypes.data, idf.ctypes.data, 2)
    assert N == 4096 * 4095 and _score(emu, tf, N, tf, N, idf) == (N * N, 1.0)
    rng = np.random.default_rng(6)
    idf = rng.integers(0, 4096, 97).astype(np.uint16)
    for _ in range(200):
        a, b = rng.integers(0, 40, 97).astype(np.uint16), rng.integers(0, 40, 97).astype(np.uint16)
        a[rng.random(97) < 0.5] = 0
        b[rng.random(97) < 0.5] = 0
        na, nb = R.norm_of(a, idf), R.norm_of(b, idf)
        assert emu.emu_norm(a.ctypes.data, idf.ctypes.data, 97) == na
        if na and nb:
            got, want = _score(emu, a, na, b, nb, idf), R.score(a, na, b, nb, idf)
            assert got[0] == want[0] and np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64)


def test_order_random_with_ties(emu):
    rng = np.random.default_rng(9)
    for _ in range(50):
        n = int(rng.integers(1, 60))
        sc = rng.integers(0, 5, n).astype(np.float64) / 4.0                    # many equal scores, many gated
        bits = np.ascontiguousarray(sc.view(np.uint64))
        K = int(rng.integers(1, 33))
        out = np.zeros(K, np.int32)
        count = emu.emu_topk(bits.ctypes.data, n, K, out.ctypes.data)
        want = sorted((i for i in range(n) if sc[i] > 0), key=lambda i: (-sc[i], i))[:K]
        assert count == len(want) and out.tolist() == want + [-1] * (K - len(want))
