"""Place recognition through the C++ adapters on the GPU (aria_hip/HipPlaceIndex.hpp, HipLoopDetector::setPlaceIndex) and the
driver flags euroc_frontend --loop --loop-bow V [--loop-bow-top K] [--loop-bow-vocab FILE] [--loop-capacity N]."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_cpp_bow_selftest(aria, tmp_path):
    """tests/cpp/bow_selftest.cpp: generated descriptor lists, a place is 300 random descriptors and a view of it 200 of them with 8
    flipped bits each.

    - the adapter trains 256 words on one view of 40 places, fills the index with a second and places all 40 third views first;
      a saved and reloaded vocabulary gives the same hits;
    - a detector that was told setPlaceIndex(nullptr) gives the candidates and detect() results of one that never heard of it;
    - a walk of 1200 keyframes whose last six see the places of the first six again: with an index (top_k 10) and a capacity of
      2000 all six loops are found, to the right keyframes; a detector of capacity 500 without an index finds none, because the
      keyframes left its database 700 keyframes ago. That is today's break, asserted as such. Six queries mid-walk, where
      nothing was seen before, find nothing."""
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "bow_selftest.cpp")
    exe = os.path.join(ROOT, "build", "bow_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe, str(tmp_path / "selftest.bow")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    kv = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.stdout.splitlines() if l.strip() and l.split()[0] != "DONE"}
    before, words, run, size, right, same, last_id = kv["adapter"]
    assert before == 0 and words == 256 and 1 <= run <= 10 and size == 40 and right == 40 and same == 1 and last_id == 39
    equal, loops, counts_equal = kv["plain_equal"]
    assert equal == 1 and loops >= 1 and counts_equal == 1
    run, n_with, n_index, n_without, found, right, found_without, false_with, queries, candidates = kv["walk"]
    assert 1 <= run <= 10 and n_with == n_index == 1200 and n_without == 500
    assert found == right == 6 and found_without == 0 and false_with == 0
    assert queries == 12 and 6 <= candidates <= 10 * queries                  # at most top_k exact checks per query, not 1200


def test_euroc_frontend_loop_bow_flag(aria, tmp_path):
    """The driver flags' plumbing, once, on the synthetic image sequence: --pose is untouched by the flag, the `loop bow` line is
    printed, the vocabulary file is written by the first run and loaded by the second with the same output, and --loop-bow
    without --loop is refused with a message that names --loop. Nothing about retrieval: that is test_cpp_bow_selftest's."""
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 6, w=640, h=480)
    exe = os.path.join(PKG, "euroc_frontend")
    t1, t2, t3, vocab = (str(tmp_path / n) for n in ("a.txt", "b.txt", "c.txt", "vocab.bow"))
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", t1, "--loop"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    flags = ["--loop", "--loop-bow", "64", "--loop-bow-top", "5", "--loop-bow-vocab", vocab, "--loop-capacity", "800"]
    first = subprocess.run([exe, str(tmp_path), "1000", "--pose", t2] + flags, capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, first.stdout + first.stderr
    assert open(t1, "rb").read() == open(t2, "rb").read()
    assert os.path.getsize(vocab) == 16 + 64 * 34
    second = subprocess.run([exe, str(tmp_path), "1000", "--pose", t3] + flags, capture_output=True, text=True, timeout=300)
    assert second.returncode == 0, second.stdout + second.stderr
    assert open(t1, "rb").read() == open(t3, "rb").read()
    lines = [[l.split() for l in r.stdout.splitlines() if l.startswith("loop bow")] for r in (first, second)]
    assert len(lines[0]) == len(lines[1]) == 1, first.stdout
    a, b = lines[0][0], lines[1][0]
    print(" ".join(a), "|", " ".join(b))
    assert a[2:4] == ["words", "64"] and a[4] == "iterations" and int(a[5]) >= 1 and b[5] == "0"      # trained, then loaded
    assert a[6:] == b[6:] and a[6] == "entries" and a[8] == "queries" and a[10] == "candidates"
    keyframes = [[l for l in r.stdout.splitlines() if l.startswith("keyframes ")] for r in (first, second)]
    assert keyframes[0] == keyframes[1] and len(keyframes[0]) == 1
    assert int(a[7]) == int(keyframes[0][0].split()[1])                         # every keyframe has its bag
    bad = subprocess.run([exe, str(tmp_path), "1000", "--pose", t2, "--loop-bow", "64"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--loop" in bad.stderr
