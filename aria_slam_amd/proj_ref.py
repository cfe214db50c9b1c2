"""NumPy restatement of guided matching (include/aria_orb_hip.h, "guided matching"; kernels in csrc/proj_search.hip). The
reference project has no such code, so this file IS the definition: the device is held to it bit for bit -- the projection is
taken in np.float64 in the header's order, every window test in np.float32 as written, and the integer steps are exact.

Also the exact scene of the tests: with fx = fy = 256, cx = 160, cy = 120, the pose [I|0] and a landmark at
X = ((u - cx) / 64, (v - cy) / 64, 4), an integer pixel (u, v) projects exactly (every product and quotient is a dyadic
rational far inside fp64 and fp32), so expected records can be written down from the construction alone."""
import numpy as np

from ._lib import KP_DTYPE, MAP_POINT_DTYPE, PNP_CORR_DTYPE, PROJ_LANDMARK_DTYPE, PROJ_OBS_DTYPE, PROJ_PAIR_DTYPE

EUROC_K = (458.654, 457.296, 367.215, 248.375)
# radius_px, ratio, th_hamming, max_octave_diff: ORB-SLAM's published tracking constants, not tuned on a recording here
DEFAULTS = dict(K=EUROC_K, min_depth=0.1, radius_px=15.0, ratio=0.9, th_hamming=100, max_octave_diff=1)
VISIBLE, CANDIDATES, ACCEPTED, WON = 1, 2, 4, 8
MAX_KP, MAX_LAND = 8192, 1 << 20
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_F = np.float32

EXACT_K = (256.0, 256.0, 160.0, 120.0)
EXACT_Z = 4.0
IDENTITY_POSE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def level_scales():
    """scale[o] of aria_orb_level_info: (float)pow((double)1.2f, o)."""
    return np.array([_F(float(_F(1.2)) ** o) for o in range(8)], np.float32)


def not_visible_obs(n):
    obs = np.zeros(n, PROJ_OBS_DTYPE)
    obs["kp_idx"] = obs["hamming"] = obs["second"] = -1
    return obs


def _config(cfg):
    return dict(DEFAULTS, **(cfg or {}))


def project(pose, X, octave, cfg, width, height):
    """Rule 1 for one landmark: (u, v, visible) with u, v np.float32 (0 when not visible)."""
    c = _config(cfg)
    fx, fy, cx, cy = (np.float64(v) for v in c["K"])
    P = np.asarray(pose, np.float64).reshape(12)
    X = np.asarray(X, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        xc = [((P[4 * r] * X[0] + P[4 * r + 1] * X[1]) + P[4 * r + 2] * X[2]) + P[4 * r + 3] for r in range(3)]
        if not (int(octave) >= 0) or not (xc[2] > np.float64(c["min_depth"])):
            return _F(0), _F(0), False
        u = _F(fx * xc[0] / xc[2] + cx)
        v = _F(fy * xc[1] / xc[2] + cy)
        if not (u >= _F(0) and u < _F(width) and v >= _F(0) and v < _F(height)):
            return _F(0), _F(0), False
    return u, v, True


def search_ref(pose, kp, desc, landmarks, cfg, width, height, first=0):
    """One valid frame: every landmark of `landmarks` (PROJ_LANDMARK_DTYPE; array index first + i) against the frame's
    keypoints. Returns (obs: PROJ_OBS_DTYPE per landmark, corr: PNP_CORR_DTYPE, pairs: PROJ_PAIR_DTYPE), the last two in
    ascending i."""
    c = _config(cfg)
    scale = level_scales()
    k = np.ascontiguousarray(kp).view(KP_DTYPE).reshape(-1)
    d = np.asarray(desc, np.uint8).reshape(-1, 32)
    lm = np.ascontiguousarray(landmarks).view(PROJ_LANDMARK_DTYPE).reshape(-1)
    assert len(d) == len(k) and len(k) <= MAX_KP and len(lm) <= MAX_LAND
    obs = not_visible_obs(len(lm))
    xk, yk = k["x"], k["y"]
    ok_clamped = np.clip(k["octave"].astype(np.int64), 0, 7)
    radius, ratio, th = _F(c["radius_px"]), _F(c["ratio"]), int(c["th_hamming"])
    claims = {}                                                                  # keypoint -> (hamming, i) of its best claim
    for i in range(len(lm)):
        u, v, vis = project(pose, lm["X"][i], lm["octave"][i], c, width, height)
        if not vis:
            continue
        o = obs[i]
        o["u"], o["v"], o["flags"] = u, v, VISIBLE
        oi = min(max(int(lm["octave"][i]), 0), 7)
        r = radius * scale[oi]                                                   # fp32 product
        with np.errstate(invalid="ignore", over="ignore"):
            cand = (np.abs(ok_clamped - oi) <= int(c["max_octave_diff"])) & (np.abs(xk - u) <= r) & (np.abs(yk - v) <= r)
        idx = np.flatnonzero(cand)
        if len(idx) == 0:
            continue
        dist = _POP[d[idx] ^ lm["desc"][i]].sum(axis=1)
        b = int(np.argmin(dist))                                                 # ties: lowest k
        ham = int(dist[b])
        second = int(np.delete(dist, b).min()) if len(idx) > 1 else -1
        o["hamming"], o["second"], o["flags"] = ham, second, VISIBLE | CANDIDATES
        if ham >= th or (second >= 0 and not (_F(ham) < ratio * _F(second))):
            continue
        o["flags"] |= ACCEPTED
        kk = int(idx[b])
        o["kp_idx"] = kk                                                         # provisional: kept by the winner alone
        if kk not in claims or (ham, i) < claims[kk]:
            claims[kk] = (ham, i)
    won = []
    for i in range(len(lm)):
        o = obs[i]
        if o["flags"] & ACCEPTED:
            kk = int(o["kp_idx"])
            if claims[kk] == (int(o["hamming"]), i):
                o["flags"] |= WON
                won.append(i)
            else:
                o["kp_idx"] = -1
    corr = np.zeros(len(won), PNP_CORR_DTYPE)
    pairs = np.zeros(len(won), PROJ_PAIR_DTYPE)
    for j, i in enumerate(won):
        kk = int(obs["kp_idx"][i])
        corr[j]["X"] = lm["X"][i]
        corr[j]["u"], corr[j]["v"] = xk[kk], yk[kk]
        pairs[j]["landmark"], pairs[j]["keypoint"] = first + i, kk
    return obs, corr, pairs


def frame_valid(pose, n, kp_stride, first, count, land_cap, n_landmarks):
    return bool(0 <= n <= kp_stride and first >= 0 and 0 <= count <= land_cap and first + count <= n_landmarks and
                np.isfinite(np.asarray(pose, np.float64)).all())


def search_frame_ref(pose, kp, desc, n, kp_stride, landmarks, first, count, land_cap, cfg, width, height):
    """One frame of a batch with the header's validity rules. kp / desc: the frame's kp_stride slots (only the first n are
    read, and none when the frame is invalid); landmarks: the whole array. Returns (obs: land_cap records, corr, pairs,
    valid)."""
    lm = np.ascontiguousarray(landmarks).view(PROJ_LANDMARK_DTYPE).reshape(-1)
    obs = not_visible_obs(land_cap)
    if not frame_valid(pose, n, kp_stride, first, count, land_cap, len(lm)):
        return obs, np.zeros(0, PNP_CORR_DTYPE), np.zeros(0, PROJ_PAIR_DTYPE), False
    k = np.ascontiguousarray(kp).view(KP_DTYPE).reshape(-1)[:n]
    d = np.asarray(desc, np.uint8).reshape(-1, 32)[:n]
    o, corr, pairs = search_ref(pose, k, d, lm[first:first + count], cfg, width, height, first=first)
    obs[:count] = o
    return obs, corr, pairs, True


def search_triple_loop(pose, kp, desc, landmarks, cfg, width, height):
    """The rules as a literal loop over landmarks and keypoints and a third over the claims: obs only. For small cases."""
    c = _config(cfg)
    scale = level_scales()
    k = np.ascontiguousarray(kp).view(KP_DTYPE).reshape(-1)
    d = np.asarray(desc, np.uint8).reshape(-1, 32)
    lm = np.ascontiguousarray(landmarks).view(PROJ_LANDMARK_DTYPE).reshape(-1)
    obs = not_visible_obs(len(lm))
    best = [-1] * len(lm)
    for i in range(len(lm)):
        u, v, vis = project(pose, lm["X"][i], lm["octave"][i], c, width, height)
        if not vis:
            continue
        oi = min(max(int(lm["octave"][i]), 0), 7)
        r = _F(c["radius_px"]) * scale[oi]
        dists = []
        for j in range(len(k)):
            oj = min(max(int(k["octave"][j]), 0), 7)
            with np.errstate(invalid="ignore", over="ignore"):
                if abs(oj - oi) <= c["max_octave_diff"] and np.abs(k["x"][j] - u) <= r and np.abs(k["y"][j] - v) <= r:
                    dists.append((sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(d[j], lm["desc"][i])), j))
        ham = second = -1
        flags = VISIBLE
        if dists:
            flags |= CANDIDATES
            dists.sort()
            ham, best[i] = dists[0]
            second = dists[1][0] if len(dists) > 1 else -1
            if ham < c["th_hamming"] and (second < 0 or _F(ham) < _F(c["ratio"]) * _F(second)):
                flags |= ACCEPTED
        obs[i] = (u, v, -1, ham, second, flags)
    for i in range(len(lm)):
        if not obs["flags"][i] & ACCEPTED:
            continue
        rivals = [(int(obs["hamming"][j]), j) for j in range(len(lm)) if obs["flags"][j] & ACCEPTED and best[j] == best[i]]
        if min(rivals)[1] == i:
            obs["flags"][i] |= WON
            obs["kp_idx"][i] = best[i]
    return obs


def landmarks_from_map_ref(arena, size, first, max_count, pair_base, view, kp, desc, n, kp_stride, n_slots):
    """The join: arena (MAP_POINT_DTYPE, `size` points of it valid) -> (landmarks: max_count records, count, invalid).
    kp (n_slots, kp_stride) KP_DTYPE, desc (n_slots, kp_stride, 32), n (n_slots,)."""
    a = np.ascontiguousarray(arena).view(MAP_POINT_DTYPE).reshape(-1)
    size = min(max(int(size), 0), len(a))
    cnt = max(min(first + max_count, size) - first, 0)
    out = np.zeros(max_count, PROJ_LANDMARK_DTYPE)
    out["octave"] = -1
    out["source"] = -1
    k = np.ascontiguousarray(kp).view(KP_DTYPE).reshape(-1, kp_stride)
    d = np.asarray(desc, np.uint8).reshape(-1, kp_stride, 32)
    invalid = False
    for j in range(cnt):
        pt = a[first + j]
        out[j]["source"] = first + j
        s = int(pt["pair"]) - pair_base
        idx = int(pt["idx1"] if view == 1 else pt["idx2"])
        if not (0 <= s < n_slots) or not (0 <= int(n[s]) <= kp_stride) or not (0 <= idx < int(n[s])):
            invalid = True
            continue
        out[j]["X"] = pt["X"]
        out[j]["desc"] = d[s, idx]
        out[j]["octave"] = k[s, idx]["octave"]
    return out, cnt, invalid


# ---- the exact scene ---------------------------------------------------------------------------------------------------
def exact_point(u, v, z=EXACT_Z):
    """The world point that the pose [I|0] and EXACT_K project exactly onto the pixel (u, v) (multiples of 1/64 at z = 4)."""
    return ((u - EXACT_K[2]) * z / EXACT_K[0], (v - EXACT_K[3]) * z / EXACT_K[1], z)


def make_landmark(u, v, desc, octave=0, source=0, z=EXACT_Z):
    lm = np.zeros(1, PROJ_LANDMARK_DTYPE)
    lm["X"][0] = exact_point(u, v, z)
    lm["desc"][0] = desc
    lm["octave"], lm["source"] = octave, source
    return lm


def make_keypoint(x, y, octave=0):
    k = np.zeros(1, KP_DTYPE)
    k["x"], k["y"], k["octave"] = x, y, octave
    k["size"], k["angle"], k["response"] = 31.0, 0.0, 1.0
    return k


def flip_bits(desc, n, start=0):
    """desc with n bits flipped, from bit `start` on."""
    out = np.array(desc, np.uint8).copy()
    for b in range(start, start + n):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def random_descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)
