"""NumPy restatement of the sparse stereo stage (include/aria_orb_hip.h, "sparse stereo"; kernels in
csrc/stereo_match.hip). The reference project has no stereo code, so this file IS the definition: the device is held to it
bit for bit -- every fp32 step below is taken in np.float32 in the header's order, every fp64 step of the scale in the
header's order, and the integer steps are exact.

Inputs are rectified (row-aligned) image pairs; rectification / undistortion is not part of the stage: see aria_rect_*
(rectify_ref.py).

Also the synthetic rectified scene of the tests: a left image of random rectangles and a right view shifted by a known
disparity per row."""
import numpy as np

from ._lib import KP_DTYPE, MATCH_DTYPE, STEREO_OBS_DTYPE, STEREO_SCALE_DTYPE

EUROC_K = (458.654, 457.296, 367.215, 248.375)
DEFAULTS = dict(K=EUROC_K, baseline=0.110, min_disparity=0.0, max_disparity=None, th_hamming=75, sad_half_window=5,
                sad_slide=5, band_factor=2.0, max_octave_diff=1, median_factor=2.1, min_scale_matches=5)
MIN_DISPARITY_CLAMP = np.float32(0.01)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_F = np.float32


def level_scales():
    """scale[o] of aria_orb_level_info: (float)pow((double)1.2f, o)."""
    return np.array([_F(float(_F(1.2)) ** o) for o in range(8)], np.float32)


def unmatched_obs(n):
    obs = np.zeros(n, STEREO_OBS_DTYPE)
    obs["right_idx"] = -1
    obs["depth"] = -1.0
    return obs


def _config(cfg):
    c = dict(DEFAULTS, **cfg)
    if c["max_disparity"] is None:
        c["max_disparity"] = c["K"][0]
    return c


def best_candidates(kp_l, desc_l, kp_r, desc_r, **cfg):
    """Step 1 for every left keypoint: (right index or -1 without a candidate, its Hamming distance). The threshold is not
    applied here."""
    c = _config(cfg)
    scale = level_scales()
    kl, kr = np.asarray(kp_l).view(KP_DTYPE).reshape(-1), np.asarray(kp_r).view(KP_DTYPE).reshape(-1)
    dl = np.asarray(desc_l, np.uint8).reshape(-1, 32)
    dr = np.asarray(desc_r, np.uint8).reshape(-1, 32)
    best = np.full(len(kl), -1, np.int32)
    dist = np.zeros(len(kl), np.int32)
    if len(kr) == 0:
        return best, dist
    xr, yr, orr = kr["x"], kr["y"], kr["octave"].astype(np.int64)
    band = _F(c["band_factor"]) * scale[np.clip(orr, 0, 7)]                      # fp32 product per right keypoint
    for i in range(len(kl)):
        xl, yl, ol = kl["x"][i], kl["y"][i], int(kl["octave"][i])
        ok = np.abs(orr - ol) <= c["max_octave_diff"]
        ok &= np.abs(yr - yl) <= band
        ok &= (xl - _F(c["max_disparity"]) <= xr) & (xr <= xl - _F(c["min_disparity"]))
        idx = np.flatnonzero(ok)
        if len(idx) == 0:
            continue
        d = _POP[dr[idx] ^ dl[i]].sum(axis=1)
        k = int(np.argmin(d))                                                    # ties: lowest j
        best[i], dist[i] = idx[k], d[k]
    return best, dist


def sad_slide(img_l, img_r, ul, vl, ur, w, L):
    """Step 2: SAD(inc) for inc in [-L, L] as an int array, or None when a window leaves the image."""
    H, W = img_l.shape
    if ul - w < 0 or ul + w > W - 1 or vl - w < 0 or vl + w > H - 1 or ur - L - w < 0 or ur + L + w > W - 1:
        return None
    a = img_l[vl - w:vl + w + 1, ul - w:ul + w + 1].astype(np.int64)
    out = np.zeros(2 * L + 1, np.int64)
    for k, inc in enumerate(range(-L, L + 1)):
        b = img_r[vl - w:vl + w + 1, ur + inc - w:ur + inc + w + 1].astype(np.int64)
        out[k] = np.abs(a - b).sum()
    return out


def stereo_match_ref(img_l, img_r, kp_l, desc_l, kp_r, desc_r, **cfg):
    """One rectified pair. Returns (obs: STEREO_OBS_DTYPE per left keypoint, matches: MATCH_DTYPE in ascending left index)."""
    c = _config(cfg)
    fx, fy, cx, cy = (_F(v) for v in c["K"])
    fb = fx * _F(c["baseline"])                                                  # formed once in fp32
    mind, maxd = _F(c["min_disparity"]), _F(c["max_disparity"])
    w, L = int(c["sad_half_window"]), int(c["sad_slide"])
    img_l, img_r = np.asarray(img_l, np.uint8), np.asarray(img_r, np.uint8)
    kl, kr = np.asarray(kp_l).view(KP_DTYPE).reshape(-1), np.asarray(kp_r).view(KP_DTYPE).reshape(-1)
    obs = unmatched_obs(len(kl))
    best, dist = best_candidates(kl, desc_l, kr, desc_r, **cfg)
    for i in range(len(kl)):
        j = int(best[i])
        if j < 0 or dist[i] >= c["th_hamming"]:
            continue
        xl, yl = kl["x"][i], kl["y"][i]
        ul, vl, ur = int(np.rint(xl)), int(np.rint(yl)), int(np.rint(kr["x"][j]))   # round-half-even
        sad = sad_slide(img_l, img_r, ul, vl, ur, w, L)
        if sad is None:
            continue
        k = int(np.argmin(sad))                                                  # ties: lowest inc
        if k == 0 or k == 2 * L:
            continue
        d1, d2, d3 = int(sad[k - 1]), int(sad[k]), int(sad[k + 1])
        den = 2 * (d1 + d3 - 2 * d2)
        if den == 0:
            continue
        delta = _F(d1 - d3) / _F(den)
        disp = _F(ul - ur - (k - L)) - delta
        if not (mind <= disp < maxd):
            continue
        disp = max(disp, MIN_DISPARITY_CLAMP)
        depth = fb / disp
        o = obs[i]
        o["u_right"] = xl - disp
        o["disparity"] = disp
        o["depth"] = depth
        o["X"] = (xl - cx) * depth / fx
        o["Y"] = (yl - cy) * depth / fy
        o["right_idx"], o["hamming"], o["sad"] = j, dist[i], d2
    kept = np.flatnonzero(obs["right_idx"] >= 0)
    if len(kept):
        med = int(np.sort(obs["sad"][kept])[len(kept) // 2])
        drop = kept[obs["sad"][kept].astype(np.float32) > _F(c["median_factor"]) * _F(med)]
        obs[drop] = unmatched_obs(1)[0]
    kept = np.flatnonzero(obs["right_idx"] >= 0)
    m = np.zeros(len(kept), MATCH_DTYPE)
    m["query_idx"], m["train_idx"], m["distance"] = kept, obs["right_idx"][kept], obs["hamming"][kept]
    return obs, m


def stereo_scale_ref(pose, mask, matches, obs_query, obs_train, query_is_first=True, min_scale_matches=5):
    """Metric scale of one relative pose (x2 ~ R x1 + t, |t| = 1): the median over the usable matches of t . (X2 - R X1)
    with X1 / X2 the stereo points of views 1 / 2. pose: a POSE_RESULT_DTYPE record or (R, t, valid); mask: per-match
    bytes or None. Returns a STEREO_SCALE_DTYPE record."""
    out = np.zeros((), STEREO_SCALE_DTYPE)
    out["scale"] = 1.0
    if isinstance(pose, tuple):
        R, t, valid = pose
    else:
        R, t, valid = pose["R"], pose["t"], pose["valid"]
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    if not int(valid):
        return out
    m = np.asarray(matches).view(MATCH_DTYPE).reshape(-1)
    oq, ot = np.asarray(obs_query).view(STEREO_OBS_DTYPE).reshape(-1), np.asarray(obs_train).view(STEREO_OBS_DTYPE).reshape(-1)
    use = np.ones(len(m), bool) if mask is None else (np.asarray(mask).reshape(-1)[:len(m)] != 0)
    a, b = oq[m["query_idx"]], ot[m["train_idx"]]
    o1, o2 = (a, b) if query_is_first else (b, a)
    use &= (o1["right_idx"] >= 0) & (o2["right_idx"] >= 0)
    o1, o2 = o1[use], o2[use]
    X1 = [o1[k].astype(np.float64) for k in ("X", "Y", "depth")]
    X2 = [o2[k].astype(np.float64) for k in ("X", "Y", "depth")]
    d = [X2[r] - (R[r, 0] * X1[0] + R[r, 1] * X1[1] + R[r, 2] * X1[2]) for r in range(3)]
    s = t[0] * d[0] + t[1] * d[1] + t[2] * d[2]
    n = len(s)
    out["n_used"] = n
    if n < min_scale_matches or n == 0:
        return out
    scale = np.sort(s)[n // 2]
    if not scale > 0:
        return out
    out["scale"], out["valid"] = scale, 1
    return out


def stereo_scene(seed, W, H):
    """Float left image: random rectangles on gray 110 plus N(0, 2) noise."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W)) + 110
    for _ in range(W * H // 350):
        x, y = rng.integers(0, W), rng.integers(0, H)
        w, h = rng.integers(4, 30, 2)
        img[y:y + h, x:x + w] = rng.integers(20, 236)
    return img + rng.normal(0, 2, img.shape)


ROW_DISPARITIES = (7.0, 19.5, 42.25)


def row_disparity(H):
    """True disparity of every row: 7.0, 19.5 and 42.25 px in the top, middle and bottom thirds."""
    d = np.empty(H)
    d[:H // 3], d[H // 3:2 * H // 3], d[2 * H // 3:] = ROW_DISPARITIES
    return d


def stereo_pair(seed, W, H):
    """(left u8, right u8, row disparities): I_R(y, x) = I_L(y, x + d[y]), bilinear, edge-clamped; both rounded and clipped."""
    left = stereo_scene(seed, W, H)
    d = row_disparity(H)
    xs = np.arange(W)[None, :] + d[:, None]
    x0 = np.floor(xs)
    f = xs - x0
    i0 = np.clip(x0.astype(np.int64), 0, W - 1)
    i1 = np.clip(x0.astype(np.int64) + 1, 0, W - 1)
    rows = np.arange(H)[:, None]
    right = (1 - f) * left[rows, i0] + f * left[rows, i1]
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)   # noqa: E731
    return to_u8(left), to_u8(right), d
