"""The case table of the absolute pose stage (aria_pnp_*), in the manner of tests/ransac_cases.py: shared by the CPU tests
(tests/test_pnp_host.py pins what the table covers, with the restatement alone), the GPU tests (tests/test_gpu_pnp.py: the
device against pnp_ref.estimate over the whole table) and tools/pnp_gap.py (the tolerance table). A plain module.

A case is Case(scene, n, outliers, noise_px, motion, H, seed, pair_base, threshold_px, K, refine_iters, copies, offset,
planar): the scene is pnp_ref.synth_pnp(scene, n, motion, outliers, noise_px) in the camera K, the world frame moved by
`offset` along (1, 1, 1) / sqrt(3); `copies` is the share of the correspondences (the last ones) that are made copies of
correspondence 0 -- a sample that holds two copies has exact zero pivots and is invalid on both sides, which moves the first
valid hypothesis, the winner of a noise-free scene, up; copies = 1 leaves no valid hypothesis at all. planar puts every point
on one plane: the 6-point DLT's known limit, valid = 0.

BAND is the relative band around the inlier threshold inside which a point counts as undecided, as in ransac_cases.py."""
import collections
import functools

import numpy as np

from aria_slam_amd import fund_ref as F
from aria_slam_amd import pnp_ref as N
from aria_slam_amd import pose_ref as P

BAND = 1e-3
EUROC = P.EUROC_K
LOOP = F.REFERENCE_LOOP_K
HIGH_SEED = 0xFEDCBA9876543210
TILE = 2048                                # points per LDS tile of k_pnp_score

Case = collections.namedtuple("Case", "scene n outliers noise_px motion H seed pair_base threshold_px K refine_iters copies "
                                      "offset planar")


def motion(k):
    """Four world-to-camera poses: the scene lies 2-20 units in front of the camera whatever the pose."""
    R, t = [(np.eye(3), [0.0, 0.0, 0.0]), (P.rot([0, 1, 0], 15), [0.5, 0.0, 1.0]), (P.rot([0.3, 1, 0.2], 25), [-1.0, 0.3, 2.0]),
            (P.rot([1, 0.2, -0.4], 40), [3.0, -2.0, 0.5])][k % 4]
    return R, np.asarray(t, np.float64)


def case_id(c):
    return "s%d-n%d-o%g-z%g-m%d-H%d-seed%x-pb%d-thr%g-%s-it%d-c%g-off%g%s" % (
        c.scene, c.n, c.outliers, c.noise_px, c.motion, c.H, c.seed, c.pair_base, c.threshold_px,
        "euroc" if c.K == EUROC else "loop", c.refine_iters, c.copies, c.offset, "-planar" if c.planar else "")


def scene(c):
    """(corr, truth, R_true, t_true) of a case."""
    R, t = motion(c.motion)
    w, h = (752, 480) if c.K == EUROC else (640, 360)
    off = np.full(3, c.offset / np.sqrt(3.0))
    corr, truth, Rt, tt = N.synth_pnp(c.scene, max(c.n, 1), R, t, c.outliers, c.noise_px, c.K, w, h, offset=off, planar=c.planar)
    corr, truth = corr[:c.n].copy(), truth[:c.n]
    k = int(round(c.n * c.copies))
    if k:
        corr[c.n - k:] = corr[0]
    return corr, truth, Rt, tt


def _c(scene, n, outliers, motion, H, seed=0, pair_base=0, thr=2.0, K=EUROC, noise=0.5, iters=5, copies=0.0, offset=0.0,
       planar=False):
    return Case(scene, n, outliers, noise, motion, H, seed, pair_base, thr, K, iters, copies, offset, planar)


HI = HIGH_SEED
PNP_CASES = [
    # the small-input gate
    _c(1, 6, 0.0, 0, 64, noise=0.05),
    _c(2, 7, 0.0, 1, 64, seed=3, noise=0.05, K=LOOP),
    _c(3, 7, 0.0, 2, 1024, seed=HI, pair_base=1000000, noise=0.0),
    # mid sizes
    _c(4, 40, 0.2, 3, 320),
    _c(5, 40, 0.3, 0, 64, pair_base=5, thr=8.0, K=LOOP),
    _c(6, 40, 0.5, 1, 1024, seed=3, pair_base=1000000),
    _c(7, 150, 0.0, 2, 320, K=LOOP),
    _c(8, 150, 0.4, 3, 1024, seed=HI, thr=0.5),
    _c(9, 600, 0.0, 0, 320, seed=3, pair_base=1000000, thr=0.5),
    _c(280, 600, 0.4, 1, 1024, pair_base=5),
    _c(11, 600, 0.5, 2, 64, pair_base=1000000, thr=8.0, K=LOOP),
    # around the 2048-point LDS tile of the scoring kernel, and the largest list
    _c(12, TILE - 1, 0.2, 3, 320, pair_base=5),
    _c(13, TILE - 1, 0.0, 0, 64, seed=HI, thr=8.0, K=LOOP),
    _c(14, TILE, 0.0, 1, 320, pair_base=5, K=LOOP),
    _c(381, TILE, 0.4, 2, 64, seed=HI, pair_base=5, thr=0.5),
    _c(400, TILE + 1, 0.0, 3, 64, pair_base=1000000),
    _c(421, TILE + 1, 0.3, 0, 320, seed=3),
    _c(446, 4096, 0.1, 1, 320, seed=3, thr=0.5),
    _c(19, 300, 0.3, 2, 4096, seed=3, pair_base=5),
    # a world origin 1000 units from the scene: what the centring on X0 is for
    _c(20, 600, 0.3, 3, 320, seed=3, offset=1000.0),
    # no refinement: the result is the winner as scored
    _c(21, 150, 0.2, 0, 320, iters=0),
    # every correspondence the same: no valid hypothesis; and a coplanar scene: the DLT's known limit
    _c(22, 50, 0.0, 1, 64, copies=1.0),
    _c(23, 150, 0.0, 2, 320, planar=True),
    # tie scenes (noise-free, no outliers): every valid hypothesis counts all n, the winner is the first of them
    _c(24, 150, 0.0, 3, 1024, pair_base=3, noise=0.0, copies=0.3),
    _c(24, 150, 0.0, 3, 1024, pair_base=0, noise=0.0, copies=0.66),
    # not exact-set (with case 7): one or two points of the refined pose inside the band; the winner's own set is exact, so
    # the refinement has the same input on both sides, and the two counts that decide `refined` differ by far more
    _c(384, TILE, 0.4, 2, 64, seed=HI, pair_base=5, thr=0.5),
    _c(443, 4096, 0.1, 1, 320, seed=3, thr=0.5),
]

# The mixed launch of the batch entry point: one configuration, pair p of the launch has pair id BATCH_BASE + p.
BATCH_BASE = 7
PNP_BATCH = [_c(sc, n, 0.0 if n <= 7 else 0.2, mo, 320, seed=3, pair_base=BATCH_BASE + p, noise=0.05 if n <= 7 else 0.5)
             for p, (sc, mo, n) in enumerate([(200, 0, 300), (201, 1, 0), (202, 2, TILE - 1), (203, 3, 5), (204, 0, TILE),
                                              (205, 1, 6), (206, 2, TILE + 1), (207, 3, 40), (228, 0, 600), (209, 1, 4),
                                              (210, 2, 150)])]


# The ground-truth set of tests/test_gpu_pnp.py: the scenes at 0.5 px whose world origin lies at the scene (at 1000 units the
# translation error is the rotation error times 1000, a different number). tools/pnp_gap.py prints the restatement's
# worst error over them; the device is allowed twice that.
GT_CASES = [i for i, c in enumerate(PNP_CASES) if c.noise_px == 0.5 and c.offset == 0.0 and not c.planar and c.copies == 0.0]


# ---- what the restatement says about a case -------------------------------------------------------------------------------
def _band(ratio):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(ratio, np.float64) - 1.0) < BAND


def unambiguous(counts, band, best):
    """No other hypothesis's count plus its in-band points reaches the winner's count minus its own; an exact tie with no
    in-band point on either side is allowed after the winner (the tie scenes: the winner is the first of them)."""
    counts, band = np.asarray(counts).ravel(), np.asarray(band).ravel()
    reach = (counts >= 0) & (counts + band >= counts[best] - band[best])
    reach[best] = False
    tie = (counts == counts[best]) & (band == 0) & (band[best] == 0) & (np.arange(len(counts)) > best)
    return not (reach & ~tie).any()


@functools.lru_cache(maxsize=None)
def report(c):
    """The restatement's fp64 and extended runs of a case and what decides how the device is compared with them: ref / ext
    (pnp_ref.estimate's dicts), hyp (pnp_ref.hypotheses), band (in-band points per hypothesis), unambiguous, band_winner /
    band_refit / in_band, soft ((n,) bool: the points of either band), exact (an exact-set case)."""
    corr, truth, Rt, tt = scene(c)
    st = N.stage(corr, c.K)
    args = dict(seed=c.seed, pair=c.pair_base, n_hyp=c.H, threshold_px=c.threshold_px, refine_iters=c.refine_iters, K=c.K)
    hyp = N.hypotheses(corr, c.seed, c.pair_base, c.H, c.threshold_px, c.K, st) if c.n >= N.MIN_CORR else None
    ref = N.estimate(corr, hyp=hyp, staged=st, **args)
    ext = N.estimate(corr, hyp=hyp, staged=st, dtype=np.longdouble, **args)
    rep = dict(case=c, corr=corr, truth=truth, R_true=Rt, t_true=tt, staged=st, hyp=hyp, ref=ref, ext=ext, unambiguous=True,
               band=None, band_winner=0, band_refit=0, in_band=0, soft=np.zeros(c.n, bool), exact=True)
    if hyp is None or not ref["valid"]:
        return rep
    _idx, R32, t032, counts = hyp
    thr2 = N.threshold2(c.threshold_px, c.K)
    live = np.flatnonzero(counts >= 0)
    band = np.zeros(c.H, np.int64)
    for a in range(0, len(live), 256):
        sel = live[a:a + 256]
        band[sel] = _band(N.error_ratio(R32[sel], t032[sel], st["d32"], st["xy32"], thr2)).sum(axis=1)
    rep["band"] = band
    rep["unambiguous"] = unambiguous(counts, band, ref["best_hypothesis"])
    soft = _band(N.error_ratio(ref["winner_R"], ref["winner_t0"], st["d32"], st["xy32"], thr2))[0]
    rep["band_winner"] = int(soft.sum())
    if ref["refit_R"] is not None:
        b = _band(N.error_ratio(ref["refit_R"], ref["refit_t0"], st["d32"], st["xy32"], thr2))[0]
        rep["band_refit"] = int(b.sum())
        soft = soft | b
    rep["in_band"] = int(soft.sum())
    rep["soft"] = soft
    rep["exact"] = rep["in_band"] == 0
    return rep


# ---- differences, as the tests and tools/pnp_gap.py measure them ------------------------------------------------------------
def diff(r, ext):
    """(R, t, rms_px): the largest entry difference of a result from the extended run."""
    return (float(np.abs(np.asarray(r["R"], np.longdouble) - ext["R"]).max()),
            float(np.abs(np.asarray(r["t"], np.longdouble) - ext["t"]).max()),
            float(abs(np.longdouble(r["rms_px"]) - ext["rms_px"])))


def gap(c):
    """The fp64 run against the extended run of the restatement -- the yardstick of the device's tolerance."""
    rep = report(c)
    return diff(rep["ref"], rep["ext"])


def truth_error(r, rep):
    """(rotation error in degrees, |t - t_true|, precision of the mask against the scene's inlier truth)."""
    sel = np.asarray(r["mask"]) == 1
    prec = float(rep["truth"][sel].mean()) if sel.any() else 0.0
    return (P.rotation_error_deg(np.asarray(r["R"], np.float64), rep["R_true"]),
            float(np.linalg.norm(np.asarray(r["t"], np.float64) - rep["t_true"])), prec)
