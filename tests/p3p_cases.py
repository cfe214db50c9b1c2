"""The case table of the absolute pose stage with the P3P minimal solver (aria_pnp_set_solver), in the manner of
tests/pnp_cases.py, whose scenes, band and difference measures it uses: shared by the CPU tests (tests/test_p3p_host.py pins
what the table covers, with the restatement alone), the GPU tests (tests/test_gpu_p3p.py: the device against
pnp_ref.estimate(solver="p3p") over the whole table) and tools/p3p_gap.py (the tolerance table). A plain module.

A case is pnp_cases.Case plus `collinear`: every world point moved onto one line, so that every sample fails the solver's
degeneracy test and no hypothesis is valid. planar=True, the 6-point DLT's known limit, is the case the solver exists for."""
import collections
import functools

import numpy as np

import pnp_cases as PC
from aria_slam_amd import pnp_ref as N

BAND = PC.BAND
EUROC, LOOP, HIGH_SEED, TILE = PC.EUROC, PC.LOOP, PC.HIGH_SEED, PC.TILE

Case = collections.namedtuple("Case", PC.Case._fields + ("collinear",))


def case_id(c):
    return PC.case_id(c) + ("-collinear" if c.collinear else "")


def scene(c):
    """(corr, truth, R_true, t_true) of a case."""
    corr, truth, Rt, tt = PC.scene(PC.Case(*c[:len(PC.Case._fields)]))
    if c.collinear and c.n:
        X = corr["X"]
        s = np.linspace(-1.0, 1.0, c.n)
        corr["X"] = X[0] + s[:, None] * (np.array([1.0, 0.5, 2.0]) + 0.0 * X[0])
    return corr, truth, Rt, tt


def _c(scene, n, outliers, motion, H, seed=0, pair_base=0, thr=2.0, K=EUROC, noise=0.5, iters=5, copies=0.0, offset=0.0,
       planar=False, collinear=False):
    return Case(scene, n, outliers, noise, motion, H, seed, pair_base, thr, K, iters, copies, offset, planar, collinear)


HI = HIGH_SEED
P3P_CASES = [
    # the small-input gate: below the solver's four, at it, and below the refinement's six
    _c(1, 3, 0.0, 0, 64, noise=0.05),
    _c(2, 0, 0.0, 1, 64),
    _c(3, 4, 0.0, 2, 64, noise=0.05),
    _c(4, 5, 0.0, 3, 64, seed=3, noise=0.05, K=LOOP),
    _c(5, 6, 0.0, 0, 320, seed=HI, pair_base=1000000, noise=0.05),
    # mid sizes
    _c(6, 40, 0.3, 1, 320, pair_base=5, thr=8.0, K=LOOP),
    _c(7, 40, 0.5, 2, 1024, seed=3, pair_base=1000000),
    # planar scenes: the DLT stage's valid = 0
    _c(8, 150, 0.0, 2, 320, planar=True),
    _c(9, 150, 0.3, 2, 320, seed=3, planar=True, K=LOOP),
    _c(10, 150, 0.0, 3, 64, seed=HI, thr=0.5, planar=True),
    _c(11, 150, 0.3, 3, 320, pair_base=5, planar=True),
    # every point on one line: no valid hypothesis
    _c(12, 150, 0.0, 1, 64, collinear=True),
    # copies of correspondence 0: none valid at share 1; a noise-free tie scene at 0.3
    _c(13, 50, 0.0, 1, 64, copies=1.0),
    _c(14, 150, 0.0, 3, 320, pair_base=3, noise=0.0, copies=0.3),
    # a world origin 1000 units from the scene
    _c(15, 300, 0.3, 3, 320, seed=3, offset=1000.0),
    # no refinement: the result is the winner as scored
    _c(16, 150, 0.2, 0, 320, iters=0),
    # the one case across the scoring kernel's 2048-point tile
    _c(17, TILE + 1, 0.2, 1, 64, seed=HI, pair_base=5),
]

BATCH_BASE = 7
P3P_BATCH = [_c(sc, n, 0.0 if n <= 6 else 0.2, mo, 320, seed=3, pair_base=BATCH_BASE + p, noise=0.05 if n <= 6 else 0.5)
             for p, (sc, mo, n) in enumerate([(300, 0, 300), (301, 1, 0), (302, 2, 3), (303, 3, 4), (304, 0, TILE - 1),
                                              (305, 1, 5), (306, 2, TILE), (307, 3, 6), (308, 0, 40), (310, 1, 150)])]

# the planar cases, and the ground-truth set: planar scenes at 0.5 px with the origin at the scene
PLANAR_CASES = [i for i, c in enumerate(P3P_CASES) if c.planar]
# the restatement's own worst error over PLANAR_CASES, measured on the CPU (tools/p3p_gap.py prints it; tests/test_p3p_host.py
# pins it): degrees, map units. The device is allowed twice that.
PLANAR_TRUTH_ERROR = (0.09255, 0.012011)


def solver_args(c):
    return dict(seed=c.seed, pair=c.pair_base, n_hyp=c.H, threshold_px=c.threshold_px, refine_iters=c.refine_iters, K=c.K,
                solver="p3p")


@functools.lru_cache(maxsize=None)
def report(c):
    """pnp_cases.report for the P3P solver: the restatement's fp64 and extended runs of a case and what decides how the device
    is compared with them, plus `slots` (the chosen candidate per hypothesis) and `ext_branches_equal` (the np.longdouble
    solver takes, on the winner's sample, the candidate tests and the choice the fp64 solver takes)."""
    corr, truth, Rt, tt = scene(c)
    st = N.stage(corr, c.K)
    args = solver_args(c)
    hyp, slots = None, None
    if c.n >= N.MIN_CORR_P3P:
        br = []
        hyp = N.hypotheses(corr, c.seed, c.pair_base, c.H, c.threshold_px, c.K, st, solver="p3p", branches=br)
        slots = br[0]
    ref = N.estimate(corr, hyp=hyp, staged=st, **args)
    ext = N.estimate(corr, hyp=hyp, staged=st, dtype=np.longdouble, **args)
    rep = dict(case=c, corr=corr, truth=truth, R_true=Rt, t_true=tt, staged=st, hyp=hyp, ref=ref, ext=ext, unambiguous=True,
               band=None, band_winner=0, band_refit=0, in_band=0, soft=np.zeros(c.n, bool), exact=True, slots=slots,
               ext_branches_equal=True)
    if hyp is None or not ref["valid"]:
        return rep
    idx, R32, t032, counts = hyp
    thr2 = N.threshold2(c.threshold_px, c.K)
    live = np.flatnonzero(counts >= 0)
    band = np.zeros(c.H, np.int64)
    for a in range(0, len(live), 256):
        sel = live[a:a + 256]
        band[sel] = PC._band(N.error_ratio(R32[sel], t032[sel], st["d32"], st["xy32"], thr2)).sum(axis=1)
    rep["band"] = band
    rep["unambiguous"] = PC.unambiguous(counts, band, ref["best_hypothesis"])
    soft = PC._band(N.error_ratio(ref["winner_R"], ref["winner_t0"], st["d32"], st["xy32"], thr2))[0]
    rep["band_winner"] = int(soft.sum())
    if ref["refit_R"] is not None:
        b = PC._band(N.error_ratio(ref["refit_R"], ref["refit_t0"], st["d32"], st["xy32"], thr2))[0]
        rep["band_refit"] = int(b.sum())
        soft = soft | b
    rep["in_band"] = int(soft.sum())
    rep["soft"] = soft
    rep["exact"] = rep["in_band"] == 0
    # the winner's sample through the solver in both precisions
    s4 = idx[ref["best_hypothesis"], :4][None]
    X, xy = st["X"][s4], st["xy"][s4]
    _R, _t, ok64, slot64, d64 = N.solve_p3p(X, xy, detail=True)
    _R, _t, okx, slotx, dx = N.solve_p3p(X, xy, dtype=np.longdouble, detail=True)
    rep["ext_branches_equal"] = bool(ok64[0] == okx[0] and slot64[0] == slotx[0] and slot64[0] == slots[ref["best_hypothesis"]]
                                     and np.array_equal(d64["alive"], dx["alive"]) and np.array_equal(d64["usable"], dx["usable"]))
    return rep


diff = PC.diff
truth_error = PC.truth_error


def gap(c):
    """The fp64 run against the extended run of the restatement -- the yardstick of the device's tolerance."""
    rep = report(c)
    return diff(rep["ref"], rep["ext"])
