"""NumPy restatement of the dense stereo stage (include/aria_orb_hip.h, "dense stereo"; kernels in csrc/dense_stereo.hip).
The reference project has no stereo code (its roadmap item H19), so this file IS the definition: the device is held to it
bit for bit. Everything up to the disparity map is integer arithmetic; the depth and the sampled records are fp32 with one
rounding per operation in the header's order.

Inputs are rectified (row-aligned) 8-bit pairs, see aria_rect_* (rectify_ref.py). The synthetic scene of the tests is the
sparse stage's, stereo_ref.stereo_pair. The aggregation is vectorised over a whole line of pixels and the disparities, so a
320x240 pair takes about a second."""
import numpy as np

from ._lib import KP_DTYPE
from .stereo_ref import EUROC_K, stereo_pair, unmatched_obs   # noqa: F401  (stereo_pair: the scene of the tests)

D = 64                                   # disparities; the only supported value
CENSUS_W, CENSUS_H = 9, 7                # 62 neighbours
OUTSIDE_COST = 64                        # C where x - d < 0
INVALID_D16 = -16
NO_KEYPOINT = 0x7FFFFFFF                 # ARIA_DENSE_NO_KEYPOINT: right_idx of a sampled record
DEFAULTS = dict(K=EUROC_K, baseline=0.110, P1=8, P2=32, uniqueness=10, lr_max_diff=1)
_F = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def _config(cfg):
    c = dict(DEFAULTS, **cfg)
    if not (1 <= c["P1"] <= c["P2"] <= 127) or not (0 <= c["uniqueness"] <= 99):
        raise ValueError("1 <= P1 <= P2 <= 127 and 0 <= uniqueness <= 99")
    return c


def popcount64(a):
    a = np.ascontiguousarray(a, np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).astype(np.uint8)
    return _POP[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.uint8)


def census(img):
    """Rule 1: one uint64 per pixel, a bit per neighbour of the 9x7 window (centre left out), set when neighbour < centre;
    coordinates clamped to the image."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    ry, rx = CENSUS_H // 2, CENSUS_W // 2
    pad = np.pad(img, ((ry, ry), (rx, rx)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    k = 0
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dy == 0 and dx == 0:
                continue
            nb = pad[ry + dy:ry + dy + H, rx + dx:rx + dx + W]
            out |= (nb < img).astype(np.uint64) << np.uint64(k)
            k += 1
    return out


def cost_volume(cen_l, cen_r):
    """Rule 2: C[y, x, d] = popcount(cenL[y, x] ^ cenR[y, x - d]), 64 where x - d < 0. uint8 [H, W, 64]."""
    H, W = cen_l.shape
    C = np.full((H, W, D), OUTSIDE_COST, np.uint8)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount64(cen_l[:, d:] ^ cen_r[:, :W - d])
    return C


def aggregate(C, P1, P2):
    """Rule 3: S = the sum of L_r over the four paths. int32 [H, W, 64]."""
    S = np.zeros(C.shape, np.int32)
    C16 = C.astype(np.int32)
    for axis in (1, 0):
        Cm, Sm = np.moveaxis(C16, axis, 0), np.moveaxis(S, axis, 0)          # [line position, pixels of the line, d], views
        n = Cm.shape[0]
        for order in (range(n), range(n - 1, -1, -1)):
            prev = None
            for i in order:
                if prev is None:
                    L = Cm[i].copy()
                else:
                    m = prev.min(axis=1, keepdims=True)
                    t = np.minimum(prev, m + P2)
                    t[:, 1:] = np.minimum(t[:, 1:], prev[:, :-1] + P1)
                    t[:, :-1] = np.minimum(t[:, :-1], prev[:, 1:] + P1)
                    L = Cm[i] + t - m
                Sm[i] += L
                prev = L
    return S


def sgm_volume(left, right, **cfg):
    """S of rule 3 for a pair, int32 [H, W, 64] (for tests)."""
    c = _config(cfg)
    return aggregate(cost_volume(census(left), census(right)), c["P1"], c["P2"])


def subpixel(s_minus, s_best, s_plus, best):
    """Rule 7 for 0 < best < 63: d16 from the three sums around the winner; the division truncates towards zero."""
    den2 = max(int(s_minus) + int(s_plus) - 2 * int(s_best), 1)
    num = (int(s_minus) - int(s_plus)) * 16 + den2
    q = abs(num) // (2 * den2)
    return 16 * int(best) + (q if num >= 0 else -q)


def right_disparity(S):
    """dR of rule 6: for every right pixel the d that minimises S(y, xr + d, d) over xr + d <= W - 1, ties to the lowest."""
    H, W, _ = S.shape
    big = np.iinfo(np.int32).max
    SR = np.full((H, W, D), big, np.int32)
    for d in range(min(D, W)):
        SR[:, :W - d, d] = S[:, d:, d]
    return SR.argmin(axis=2)


def disparity_from_volume(S, uniqueness=10, lr_max_diff=1):
    """Rules 4-7: the int16 map in 1/16 px, -16 where invalid."""
    H, W, _ = S.shape
    S = S.astype(np.int64)
    best = S.argmin(axis=2)                                                  # ties: lowest d
    yy, xx = np.mgrid[0:H, 0:W]
    sb = S[yy, xx, best]
    far = np.abs(np.arange(D)[None, None, :] - best[:, :, None]) > 1
    invalid = (far & (S * (100 - uniqueness) < (sb * 100)[:, :, None])).any(axis=2)
    if lr_max_diff >= 0:
        xr = xx - best
        dR = right_disparity(S)
        invalid |= xr < 0
        invalid |= np.abs(dR[yy, np.maximum(xr, 0)] - best) > lr_max_diff
    sm = S[yy, xx, np.maximum(best - 1, 0)]
    sp = S[yy, xx, np.minimum(best + 1, D - 1)]
    den2 = np.maximum(sm + sp - 2 * sb, 1)
    num = (sm - sp) * 16 + den2
    q = np.abs(num) // (2 * den2)
    off = np.where(num >= 0, q, -q)
    off[(best == 0) | (best == D - 1)] = 0
    d16 = 16 * best + off
    d16[invalid] = INVALID_D16
    return d16.astype(np.int16)


def dense_disparity(left, right, **cfg):
    """One rectified pair -> int16 [H, W] disparities in 1/16 px."""
    c = _config(cfg)
    return disparity_from_volume(sgm_volume(left, right, **cfg), c["uniqueness"], c["lr_max_diff"])


def _fb(K, baseline):
    return _F(K[0]) * _F(baseline)                                           # formed once in fp32


def depth_map(d16, K=EUROC_K, baseline=0.110):
    """Rule 8: fp32 depth = fb / ((float)d16 * 0.0625f), 0 where d16 <= 0."""
    d16 = np.asarray(d16, np.int16)
    disp = d16.astype(np.float32) * _F(0.0625)
    out = np.zeros(d16.shape, np.float32)
    ok = d16 > 0
    out[ok] = _fb(K, baseline) / disp[ok]
    return out


def sample(d16, kps, K=EUROC_K, baseline=0.110):
    """Rule 9: one STEREO_OBS_DTYPE record per keypoint from the disparity map."""
    d16 = np.asarray(d16, np.int16)
    H, W = d16.shape
    k = np.asarray(kps).view(KP_DTYPE).reshape(-1)
    fx, fy, cx, cy = (_F(v) for v in K)
    fb = _fb(K, baseline)
    obs = unmatched_obs(len(k))
    big = _F(1.0e6)
    for i in range(len(k)):
        x, y = k["x"][i], k["y"][i]
        if np.isnan(x) or np.isnan(y):
            continue
        u, v = int(np.rint(np.clip(x, -big, big))), int(np.rint(np.clip(y, -big, big)))   # round-half-even
        if u < 0 or u > W - 1 or v < 0 or v > H - 1 or d16[v, u] <= 0:
            continue
        disp = _F(d16[v, u]) * _F(0.0625)
        depth = fb / disp
        o = obs[i]
        o["u_right"] = x - disp
        o["disparity"] = disp
        o["depth"] = depth
        o["X"] = (x - cx) * depth / fx
        o["Y"] = (y - cy) * depth / fy
        o["right_idx"], o["hamming"], o["sad"] = NO_KEYPOINT, 0, 0
    return obs


def sample_batch(d16_maps, kp, counts, K=EUROC_K, baseline=0.110):
    """The batch call: kp [n_frames, kp_stride]; records at and beyond a frame's count are unmatched, and a count outside
    [0, kp_stride] leaves its whole frame unmatched."""
    kp = np.asarray(kp).view(KP_DTYPE)
    n, stride = kp.shape
    out = unmatched_obs(n * stride).reshape(n, stride)
    for f in range(n):
        c = int(counts[f])
        if 0 <= c <= stride:
            out[f, :c] = sample(d16_maps[f], kp[f, :c], K, baseline)
    return out


def scratch_bytes_per_pair(width, height):
    """HBM scratch the handle needs per pair in flight: two census words (16 B), the 64 partial sums of S as uint16
    (128 B) and the right view's packed minimum (4 B) per pixel."""
    return 148 * int(width) * int(height)
