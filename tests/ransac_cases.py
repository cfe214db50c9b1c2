"""The case table of the two RANSAC stages (essential matrix + recoverPose, fundamental matrix), shared by the CPU tests
(tests/test_pose_host.py, tests/test_fund_host.py: they pin what the table covers, with the restatements alone), the GPU
tests (tests/test_gpu_pose.py, tests/test_gpu_fund.py: the device against pose_ref.estimate / fund_ref.estimate over the
whole table) and tools/pose_gap.py (the tolerance table). A plain module: no fixtures, no pytest.

A case is Case(scene, n, outliers, noise_px, motion, H, seed, pair_base, threshold_px, distance_thresh, K, query_is_first,
copies): the scene is pose_ref.synth_two_view(scene, n, motion, outliers, noise_px) in the camera K; `copies` is the share
of the matches (the last ones) that are made copies of match 0 -- the tie scenes: a sample that holds two copies has exact
zero pivots and is invalid on both sides, which moves the first valid hypothesis, the winner of a noise-free scene, up.
copies = 1 leaves no valid hypothesis at all. The fundamental-matrix cases do not use distance_thresh; their K only
shapes the scene.

BAND is the relative band around the inlier threshold inside which the device's fp32 test and the restatement's fp64 test
may decide differently (the band of the existing hypothesis tests). NEAR is the relative band of the cheirality test."""
import collections
import functools

import numpy as np

from aria_slam_amd import fund_ref as F
from aria_slam_amd import pose_ref as P

BAND = 1e-3
NEAR = 1e-9
EUROC = P.EUROC_K
LOOP = F.REFERENCE_LOOP_K
HIGH_SEED = 0xFEDCBA9876543210            # the config field is a uint64

Case = collections.namedtuple("Case", "scene n outliers noise_px motion H seed pair_base threshold_px distance_thresh K "
                                      "query_is_first copies")


def motion(k):
    """The four motions of the existing pose and fundamental tests."""
    R, t = [(np.eye(3), [0, 0, 1.0]), (np.eye(3), [1.0, 0, 0]), (P.rot([0.3, 1, 0.2], 5), [1, 0.3, 1.0]),
            (P.rot([0, 1, 0], 15), [0.5, 0, 1.0])][k % 4]
    t = np.asarray(t, np.float64)
    return R, t / np.linalg.norm(t)


def case_id(c):
    return "s%d-n%d-o%g-z%g-m%d-H%d-seed%x-pb%d-thr%g-d%s-%s-%s-c%g" % (
        c.scene, c.n, c.outliers, c.noise_px, c.motion, c.H, c.seed, c.pair_base, c.threshold_px,
        "x" if c.distance_thresh is None else "%g" % c.distance_thresh, "euroc" if c.K == EUROC else "loop",
        "q1" if c.query_is_first else "t1", c.copies)


def scene(c):
    """(kp_query, kp_train, matches) of a case: view 1 is the query side of the generator whatever query_is_first says, so
    query_is_first = False estimates the reverse motion."""
    R, t = motion(c.motion)
    w, h = (752, 480) if c.K == EUROC else (640, 360)
    kq, kt, m, _truth = P.synth_two_view(c.scene, max(c.n, 1), R, t, c.outliers, c.noise_px, c.K, w, h)
    kq, kt, m = kq[:c.n], kt[:c.n], m[:c.n].copy()
    k = int(round(c.n * c.copies))
    if k:
        m["query_idx"][c.n - k:] = 0
        m["train_idx"][c.n - k:] = 0
    return kq, kt, m


# ---- the table ----------------------------------------------------------------------------------------------------------
def _p(scene, n, outliers, motion, H, seed=0, pair_base=0, thr=1.0, dist=50.0, K=EUROC, qif=True, noise=0.5, copies=0.0):
    return Case(scene, n, outliers, noise, motion, H, seed, pair_base, thr, dist, K, qif, copies)


def _f(scene, n, outliers, motion, H, seed=0, pair_base=0, thr=3.0, qif=True, noise=0.5, copies=0.0):
    return Case(scene, n, outliers, noise, motion, H, seed, pair_base, thr, None, LOOP, qif, copies)


HI = HIGH_SEED
POSE_CASES = [
    # the small-input gate; n = 9 at 0.5 px leaves the winner 4 inliers: no refit
    _p(72, 8, 0.0, 72, 64, noise=0.05, qif=False),
    _p(70, 9, 0.0, 70, 64, seed=3, noise=0.0, qif=False),
    _p(15, 9, 0.0, 2, 1024, seed=HI, pair_base=1000000, K=LOOP),
    # mid sizes
    _p(19, 40, 0.2, 3, 320, qif=False),
    _p(20, 40, 0.3, 4, 64, pair_base=5, thr=3.0, K=LOOP),
    _p(21, 40, 0.4, 5, 320, seed=3, pair_base=1000000, dist=5.0),
    _p(22, 150, 0.0, 3, 320, K=LOOP),
    _p(25, 150, 0.4, 6, 1024, seed=HI, thr=0.25, qif=False),
    _p(27, 300, 0.2, 5, 320, seed=3, pair_base=1000000, thr=3.0, K=LOOP, qif=False),
    _p(28, 300, 0.3, 6, 1024, seed=HI),
    _p(29, 300, 0.4, 7, 320, pair_base=5, thr=3.0, dist=5.0, K=LOOP),
    _p(30, 600, 0.0, 5, 320, seed=3, pair_base=1000000, thr=0.25),
    _p(32, 600, 0.3, 7, 320, pair_base=5, thr=0.25, dist=5.0, qif=False),
    _p(33, 600, 0.4, 8, 64, pair_base=1000000, K=LOOP, qif=False),
    # around the 2048-point LDS tile of the scoring kernel, and the largest list
    _p(35, 2047, 0.2, 7, 320, pair_base=5, qif=False),
    _p(34, 2047, 0.0, 6, 64, seed=HI, thr=3.0, K=LOOP, qif=False),
    _p(37, 2047, 0.4, 9, 320, seed=3, dist=5.0),
    _p(38, 2048, 0.0, 7, 320, pair_base=5, K=LOOP),
    _p(41, 2048, 0.4, 10, 64, seed=HI, pair_base=5, thr=0.25, qif=False),
    _p(42, 2049, 0.0, 8, 64, pair_base=1000000, qif=False),
    _p(46, 4096, 0.0, 9, 320, seed=3, thr=0.25),
    _p(50, 300, 0.3, 3, 4096, seed=3, pair_base=5),
    # every match the same point pair: no valid hypothesis
    _p(51, 50, 0.0, 0, 64, copies=1.0),
    # tie scenes (noise-free, no outliers): the reference's winner is hypothesis 1 and hypothesis 306
    _p(60, 150, 0.0, 3, 1024, pair_base=3, noise=0.0, copies=0.3),
    _p(60, 150, 0.0, 3, 1024, pair_base=0, noise=0.0, copies=0.66),
    # not exact-set: one or two points of the refitted E inside the band; the winner's own set is exact, so the refit is
    # the same on both sides, and the two counts that decide `refined` differ by far more than the band holds
    _p(108, 2049, 0.1, 108, 64, K=LOOP),
    _p(152, 2048, 0.3, 152, 64, seed=HI, pair_base=1000000, thr=3.0),
    _p(119, 4096, 0.3, 119, 320, seed=HI, thr=0.25, K=LOOP),
]

FUND_CASES = [
    _f(10, 15, 0.0, 0, 64, qif=False),
    _f(12, 15, 0.2, 2, 1024, seed=HI, pair_base=1000000, thr=1.0),
    _f(15, 16, 0.0, 2, 1024, seed=HI, pair_base=1000000, thr=1.0),
    _f(17, 16, 0.5, 4, 64, pair_base=5, qif=False),
    _f(18, 40, 0.0, 2, 1024, seed=HI, pair_base=1000000, qif=False),
    _f(20, 40, 0.3, 4, 64, pair_base=5, thr=1.0),
    _f(22, 150, 0.0, 3, 320, thr=1.0),
    _f(25, 150, 0.4, 6, 1024, seed=HI, qif=False),
    _f(27, 300, 0.2, 5, 320, seed=3, pair_base=1000000, qif=False),
    _f(29, 300, 0.4, 7, 320, pair_base=5, thr=1.0),
    _f(31, 600, 0.2, 6, 1024, seed=HI, thr=1.0),
    _f(32, 600, 0.3, 7, 320, pair_base=5, qif=False),
    _f(34, 2047, 0.0, 6, 64, seed=HI, qif=False),
    _f(38, 2048, 0.0, 7, 320, pair_base=5, thr=1.0),
    _f(40, 2048, 0.3, 9, 320, seed=3, qif=False),
    _f(42, 2049, 0.0, 8, 64, pair_base=1000000, qif=False),
    _f(45, 2049, 0.4, 11, 320, pair_base=1000000, thr=1.0),
    _f(48, 4096, 0.3, 11, 320, pair_base=1000000, qif=False),
    _f(50, 300, 0.3, 3, 4096, seed=3, pair_base=5),
    # every match the same point pair: every sample is collinear, no model, so the stage fails MIN_INLIERS
    _f(51, 50, 0.0, 0, 64, copies=1.0),
    # tie scenes: the reference's winner is (h, root) = (1, 1) and (293, 1)
    _f(60, 150, 0.0, 3, 1024, pair_base=3, noise=0.0, copies=0.3),
    _f(60, 150, 0.0, 3, 1024, pair_base=0, noise=0.0, copies=0.66),
    # not exact-set: one to three points of the winner inside the band
    _f(41, 2048, 0.4, 10, 64, seed=HI, pair_base=5, qif=False),
    _f(44, 2049, 0.3, 10, 64, seed=HI, pair_base=5, thr=1.0),
    _f(47, 4096, 0.2, 10, 64, seed=HI, pair_base=5, thr=1.0),
]

# The mixed launches of the batch entry points: one configuration, pair p of the launch has pair id BATCH_BASE + p. Sizes
# below the gates sit between the tile-boundary sizes. (scene, motion, n) per pair.
POSE_BATCH_BASE, FUND_BATCH_BASE = 7, 11
POSE_BATCH = [_p(sc, n, 0.0 if n <= 9 else 0.2, mo, 320, seed=3, pair_base=POSE_BATCH_BASE + p, noise=0.05 if n <= 9 else 0.5)
              for p, (sc, mo, n) in enumerate([(200, 200, 300), (203, 201, 0), (208, 204, 2047), (209, 203, 5), (216, 208, 2048),
                                               (217, 207, 8), (218, 206, 2049), (221, 207, 40), (224, 208, 600), (227, 209, 7),
                                               (230, 210, 150)])]
FUND_BATCH = [_f(sc, n, 0.0 if n <= 16 else 0.2, mo, 320, seed=HI, pair_base=FUND_BATCH_BASE + p)
              for p, (sc, mo, n) in enumerate([(201, 201, 300), (203, 201, 0), (206, 202, 2047), (209, 203, 14), (213, 205, 2048),
                                               (215, 205, 15), (218, 206, 2049), (221, 207, 40), (224, 208, 600), (227, 209, 7),
                                               (231, 211, 16)])]


# ---- what the restatement says about a case -------------------------------------------------------------------------------
def _band(err, thr2):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(err, np.float64) / float(thr2) - 1.0) < BAND


def _unambiguous(counts, band, best):
    """No other entry's count plus its in-band points reaches the winner's count minus its own; an exact tie with no
    in-band point on either side is allowed (the tie scenes: the winner is the first of them)."""
    counts, band = np.asarray(counts).ravel(), np.asarray(band).ravel()
    reach = (counts >= 0) & (counts + band >= counts[best] - band[best])
    reach[best] = False
    tie = (counts == counts[best]) & (band == 0) & (band[best] == 0) & (np.arange(len(counts)) > best)
    return not (reach & ~tie).any()


@functools.lru_cache(maxsize=None)
def pose_report(c):
    """The restatement's fp64 and extended runs of a pose case and what decides how the device is compared with them:
    ref / ext (pose_ref.estimate's dicts), unambiguous, in_band (points of the winner's and the refit's 1e-3 bands),
    near (near-cheirality points), soft ((n,) bool: the union of both), margin (the chosen candidate's count minus the best
    other), exact (an exact-set case)."""
    kq, kt, m = scene(c)
    pts = P.normalise(kq, kt, m, c.query_is_first, c.K)
    args = (c.seed, c.pair_base, c.H, c.threshold_px, c.distance_thresh, c.K)
    hyp = P.hypotheses(pts, c.seed, c.pair_base, c.H, c.threshold_px, c.K) if c.n >= 8 else None
    ref = P.estimate_points(pts, *args, hyp=hyp)
    ext = P.estimate_points(pts, *args, dtype=np.longdouble, hyp=hyp)
    rep = dict(case=c, pts=pts, ref=ref, ext=ext, unambiguous=True, in_band=0, near=0, soft=np.zeros(c.n, bool), margin=0,
               exact=True, band_winner=0, band_refit=0)
    if hyp is None or not ref["valid"]:
        return rep
    _idx, E, counts = hyp
    thr2 = P.threshold2(c.threshold_px, c.K)
    live = np.flatnonzero(counts >= 0)
    band = np.zeros(c.H, np.int64)
    band[live] = _band(P.sampson_error(E[live].astype(np.float32), pts), thr2).sum(axis=1)
    rep["unambiguous"] = _unambiguous(counts, band, ref["best_hypothesis"])
    soft = _band(P.sampson_error(ref["winner_E"], pts), thr2)[0]
    rep["band_winner"] = int(soft.sum())
    if ref["refit_E"] is not None:
        b = _band(P.sampson_error(np.asarray(ref["refit_E"], np.float64).astype(np.float32), pts), thr2)[0]
        rep["band_refit"] = int(b.sum())
        soft = soft | b
    rep["in_band"] = int(soft.sum())
    # near-cheirality points among the final inliers, under any of the four candidates
    final = (P.sampson_inliers(np.asarray(ref["E"], np.float64).astype(np.float32).ravel(), pts, thr2)[0] if ref["refined"]
             else P.sampson_inliers(ref["winner_E"], pts, thr2)[0])
    near = np.zeros(c.n, bool)
    d = c.distance_thresh
    for R, t in P.decompose_essential(ref["E"]):
        det, z1, z2 = P.depths(R, t, pts)
        with np.errstate(all="ignore"):
            nz = (np.abs(z1) <= NEAR * d) | (np.abs(z2) <= NEAR * d) | (np.abs(z1 - d) <= NEAR * d) | (np.abs(z2 - d) <= NEAR * d)
            nz |= ~np.isfinite(z1) | ~np.isfinite(z2) | (np.abs(det) <= NEAR)
        near |= nz & final
    rep["near"] = int(near.sum())
    rep["soft"] = soft | near
    g = list(ref["good"])
    rep["margin"] = g.pop(ref["candidate"]) - max(g)
    rep["exact"] = rep["in_band"] == 0 and rep["near"] == 0
    return rep


@functools.lru_cache(maxsize=None)
def fund_report(c):
    """The same for a fundamental-matrix case: ref (fund_ref.estimate's dict), unambiguous, in_band / soft (the winner's
    band), exact, and F_ext (the winning model from the extended run of solve7, or None)."""
    kq, kt, m = scene(c)
    pts = F.pixels(kq, kt, m, c.query_is_first)
    hyp = F.hypotheses(pts, c.seed, c.pair_base, c.H, c.threshold_px)
    ref = F.estimate_points(pts, c.seed, c.pair_base, c.H, c.threshold_px, hyp=hyp)
    rep = dict(case=c, pts=pts, ref=ref, unambiguous=True, in_band=0, soft=np.zeros(c.n, bool), exact=True, F_ext=None,
               matches=m)
    idx, nm, Fh, counts = hyp
    thr2 = F.threshold2(c.threshold_px)
    live = np.flatnonzero(nm > 0)
    if c.n < F.MIN_MATCHES or not len(live):
        return rep
    band = np.zeros((c.H, 3), np.int64)
    band[live] = _band(F.errors(Fh[live].reshape(-1, 9), pts), thr2).sum(axis=1).reshape(-1, 3)
    band[counts < 0] = 0
    best = int(np.argmax(counts.reshape(-1)))
    rep["unambiguous"] = _unambiguous(counts, band, best)
    if not ref["valid"]:
        # fails MIN_INLIERS: the best count with every in-band point added must still fail
        rep["unambiguous"] = bool((counts + band).max() < F.MIN_INLIERS)
        return rep
    h, k = ref["best_hypothesis"], ref["best_root"]
    rep["soft"] = _band(F.errors(Fh[h, k], pts), thr2)[0]
    rep["in_band"] = int(rep["soft"].sum())
    rep["exact"] = rep["in_band"] == 0
    Fx, nx = F.solve7(np.asarray(pts)[idx[h]][None], dtype=np.longdouble)
    if nx[0] == nm[h]:
        rep["F_ext"] = Fx[0, k].reshape(3, 3)
    return rep


def in_band_limit(n):
    return max(2, n // 200)


# ---- differences, as the tests and tools/pose_gap.py measure them -----------------------------------------------------------
def e_diff(a, b):
    """Largest entry difference of two essential matrices scaled to unit Frobenius norm, over both signs."""
    a, b = np.asarray(a, np.longdouble).ravel(), np.asarray(b, np.longdouble).ravel()
    a, b = a / np.sqrt((a * a).sum()), b / np.sqrt((b * b).sum())
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


def f_diff(a, b):
    """Largest entry difference of two fundamental matrices, each scaled by the second one's largest entry."""
    a, b = np.asarray(a, np.longdouble).ravel(), np.asarray(b, np.longdouble).ravel()
    return float(np.abs(a - b).max() / np.abs(b).max())


def rt_diff(R, t, ref):
    return (float(np.abs(np.asarray(R, np.longdouble) - ref["R"]).max()),
            float(np.abs(np.asarray(t, np.longdouble) - ref["t"]).max()))


def pose_gap(c):
    """(E, R, t): the fp64 run against the extended run of the restatement -- the yardstick of the device's tolerance."""
    rep = pose_report(c)
    r, t = rt_diff(rep["ref"]["R"], rep["ref"]["t"], rep["ext"])
    return e_diff(rep["ref"]["E"], rep["ext"]["E"]), r, t


def fund_gap(c):
    rep = fund_report(c)
    return f_diff(rep["ref"]["F"], rep["F_ext"])
