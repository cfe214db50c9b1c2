"""Batch-path k_describe against the oracle, byte for byte (keypoint records and descriptors): the shapes that exercise the
16-keypoints-per-wave form's edges. Prints one "OK <case>" line per case; exits non-zero on the first difference.

Run by tests/test_gpu_describe16.py against the product library and, through ARIA_ORB_HIP_LIBRARY + ARIA_DESC_IMPL=quad,
against the variants build's 4-keypoints-per-wave body.

  levels    : many max_features values on 320x240 pairs: per-level counts of every residue mod 16 (partial last rounds,
              single-round waves, levels of 1..17 keypoints)
  kpcap     : a batch whose kp_cap is smaller than a frame's result: counts clamped, ERRBIT_KPCAP, rows needed reported,
              the rows that fit equal the oracle's first rows
  tiestorm  : a dot grid between two ordinary frames: the arena pass (k_describe<1, true>) in the batch path
  big       : 1408x1408, 4000 keypoints (BASELINE configs[3])"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import aria_slam_amd as A  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

DEV = torch.device("cuda", 0)


def run_batch(imgs, nf, cap=None, expect_status=0):
    """extract_batch_device on `imgs`; returns (counts, kps bytes, desc, rows_needed, fast/blur kernel name)."""
    B, h, w = imgs.shape
    e = A.OrbHipExtractor(max_features=nf, max_width=w, max_height=h, max_batch=B)
    try:
        cap = e.kp_capacity() if cap is None else cap
        kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device=DEV)
        desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=DEV)
        cnt = torch.zeros((B,), dtype=torch.int32, device=DEV)
        d_img = torch.from_numpy(np.ascontiguousarray(imgs)).to(DEV)
        torch.cuda.synchronize()
        e.extract_batch_device(d_img, B, w, h, kps, desc, cnt, cap)
        status, need = 0, 0
        try:
            e.check()
        except A.AriaError as ex:
            status = ex.status
            need = e.rows_needed()
        assert status == expect_status, (status, expect_status)
        return cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy(), need, e.fast_blur_kernel()
    finally:
        e.close()


def compare(imgs, nf, want, got, rows=None):
    cnt, kps, desc = got[:3]
    for f in range(len(imgs)):
        ok, od = want[f]
        n = len(ok) if rows is None else min(rows, len(ok))
        assert cnt[f] == n, (f, cnt[f], n)
        assert kps[f, :n].tobytes() == ok[:n].tobytes(), "frame %d: keypoint records differ" % f
        assert np.array_equal(desc[f, :n], od[:n]), "frame %d: descriptors differ" % f


def case_levels():
    residues = set()
    a, b = A.synth_frame_pair(41, 320, 240)
    imgs = np.stack([a, b])
    for nf in (5, 9, 13, 17, 23, 31, 40, 57, 64, 77, 90, 101, 128, 150, 173, 199, 250, 301, 333, 400, 500, 613):
        p = O.default_params(nf)
        want = [O.orb_extract(im, p) for im in imgs]
        got = run_batch(imgs, nf)
        assert got[4] == "k_fast_blur_stream", got[4]            # the Q4 batch path (the form under test)
        compare(imgs, nf, want, got)
        for ok, _ in want:
            oct_ = np.frombuffer(ok.tobytes(), dtype=np.int32).reshape(len(ok), 6)[:, 5] if len(ok) else np.zeros(0, np.int32)
            for lv in range(8):
                c = int((oct_ == lv).sum())
                if c:
                    residues.add(c % 16)
    assert residues == set(range(16)), "level counts did not cover every residue mod 16: %s" % sorted(residues)
    print("OK levels (residues mod 16 covered)")


def case_kpcap():
    imgs = A.synth_sequence(3, 1, 640, 480)
    nf = 2000
    want = [O.orb_extract(im, O.default_params(nf)) for im in imgs]
    cap = 333                                                    # not a multiple of 4 or 16
    got = run_batch(imgs, nf, cap=cap, expect_status=-5)
    assert got[3] == max(len(w[0]) for w in want), (got[3], [len(w[0]) for w in want])
    compare(imgs, nf, want, got, rows=cap)
    print("OK kpcap")


def _dots(w, h, pitch):
    img = np.full((h, w), 50, np.uint8)
    img[pitch // 2::pitch, pitch // 2::pitch] = 255
    return img


def case_tiestorm():
    w, h, nf = 320, 240, 300
    imgs = np.stack([A.synth_frame_pair(8, w, h)[0], _dots(w, h, 7), A.synth_frame_pair(9, w, h)[1]])
    want = [O.orb_extract(im, O.default_params(nf), cap=200000) for im in imgs]
    need = max(len(x[0]) for x in want)
    got = run_batch(imgs, nf, cap=need + 5)
    assert got[4] == "k_fast_blur_stream", got[4]
    compare(imgs, nf, want, got)
    print("OK tiestorm (%d rows)" % need)


def case_big():
    W = H = 1408
    nf = 4000
    a, b = A.synth_frame_pair(12, W, H)
    imgs = np.stack([a, b])
    want = [O.orb_extract(im, O.default_params(nf)) for im in imgs]
    got = run_batch(imgs, nf)
    assert got[4] == "k_fast_blur_stream", got[4]
    compare(imgs, nf, want, got)
    print("OK big")


if __name__ == "__main__":
    A.load_library()
    O.build()
    O.lib()
    cases = sys.argv[1:] or ["levels", "kpcap", "tiestorm", "big"]
    for c in cases:
        globals()["case_" + c]()
