"""The case table of guided matching, shared by tests/test_proj_host.py (the restatement), tests/test_proj_kernel_emulation.py
(the kernels' plain arithmetic on the host) and tests/test_gpu_proj.py (the device).

Every scene is exact by construction (aria_slam_amd/proj_ref.py, "the exact scene"): fx = fy = 256, cx = 160, cy = 120, the pose
[I|0] and X = ((u - cx) / 64, (v - cy) / 64, 4) project an integer pixel exactly, so the expected records below are written down
from the construction alone, never computed by the restatement. One configuration (the defaults, r = 15 px at octave 0) and one
landmark array serve every frame, so the whole table is one batch: 320 x 240, kp_stride 320, land_cap 260."""
import functools

import numpy as np

from aria_slam_amd import proj_ref as R
from aria_slam_amd._lib import KP_DTYPE, PNP_CORR_DTYPE, PROJ_LANDMARK_DTYPE, PROJ_OBS_DTYPE, PROJ_PAIR_DTYPE

W, H = 320, 240
KP_STRIDE, LAND_CAP = 320, 260
CFG = dict(K=R.EXACT_K)                                   # every other field at its default
CHUNK = 256                                               # landmarks per workgroup of k_proj_search
ALL = R.VISIBLE | R.CANDIDATES | R.ACCEPTED | R.WON


def _obs(u, v, kp=-1, ham=-1, second=-1, flags=R.VISIBLE):
    o = np.zeros(1, PROJ_OBS_DTYPE)
    o["u"], o["v"], o["kp_idx"], o["hamming"], o["second"], o["flags"] = u, v, kp, ham, second, flags
    return o


def _hidden():
    return R.not_visible_obs(1)


class _Frame:
    def __init__(self, name, pose=None):
        self.name, self.pose = name, (R.IDENTITY_POSE.copy() if pose is None else np.asarray(pose, np.float64))
        self.kp, self.desc = [], []

    def add(self, x, y, desc, octave=0):
        self.kp.append(R.make_keypoint(x, y, octave))
        self.desc.append(np.asarray(desc, np.uint8).reshape(1, 32))
        return len(self.kp) - 1


def _finish(frame, lms, exp, first=None, count=None, n=None, valid=True, poison=None):
    kp = np.concatenate(frame.kp) if frame.kp else np.zeros(0, KP_DTYPE)
    desc = np.concatenate(frame.desc) if frame.desc else np.zeros((0, 32), np.uint8)
    return dict(name=frame.name, pose=frame.pose, kp=kp, desc=desc, n=len(kp) if n is None else n, lms=lms, exp=exp, first=first,
                count=count, valid=valid, poison=poison)


# ---- the groups of landmarks; each returns (landmarks, [frames]) ---------------------------------------------------------
def _grid(rng):
    """130 landmarks 22 x 20 px apart, random descriptors. Keypoints sit within 3 px of their landmark, so 19 px or more from
    every other one: a keypoint is a candidate of its own landmark alone."""
    pos = [(20 + 22 * (i % 13), 15 + 20 * (i // 13)) for i in range(130)]
    D = R.random_descriptors(rng, 130)
    lms = np.concatenate([R.make_landmark(u, v, D[i], source=1000 + i) for i, (u, v) in enumerate(pos)])
    off = [((i % 7) - 3, (i % 5) - 2) for i in range(130)]
    poison = (np.concatenate([R.make_keypoint(u, v) for u, v in pos]), D)      # beyond a frame's count: perfect matches nobody may read

    # 301 keypoints: a primary for every landmark (i % 40 bits flipped), a runner-up for the first 100 (60 + i % 3 bits), and 71
    # far from every window (y = 226); their order is a fixed permutation
    items = [("p", i) for i in range(130)] + [("s", i) for i in range(100)] + [("f", j) for j in range(71)]
    order = np.random.default_rng(11).permutation(len(items))
    full = _Frame("grid 301")
    where = {}
    for slot in order:
        kind, i = items[slot]
        if kind == "p":
            where[i] = full.add(pos[i][0] + off[i][0], pos[i][1] + off[i][1], R.flip_bits(D[i], i % 40))
        elif kind == "s":
            full.add(pos[i][0] - off[i][0] + 0.5, pos[i][1] + 3, R.flip_bits(D[i], 60 + i % 3, start=64))
        else:
            full.add(5 + 4 * i, 226, R.flip_bits(D[i], 1))
    exp_full = np.concatenate([_obs(pos[i][0], pos[i][1], where[i], i % 40, 60 + i % 3 if i < 100 else -1, ALL) for i in range(130)])

    empty = _Frame("grid 0")
    exp_empty = np.concatenate([_obs(u, v) for u, v in pos])

    some = _Frame("grid 64")                                                   # the primaries of landmarks 63 .. 0
    for i in range(63, -1, -1):
        some.add(pos[i][0] + off[i][0], pos[i][1] + off[i][1], R.flip_bits(D[i], i % 40))
    exp_some = np.concatenate([_obs(pos[i][0], pos[i][1], 63 - i, i % 40, -1, ALL) if i < 64 else _obs(*pos[i]) for i in range(130)])

    # a known motion: t = (0.25, -0.125, 0) moves every projection by exactly (+16, -8) px
    moved = _Frame("grid moved", pose=[1, 0, 0, 0.25, 0, 1, 0, -0.125, 0, 0, 1, 0])
    for i in range(63, -1, -1):
        moved.add(pos[i][0] + 16 + off[i][0], pos[i][1] - 8 + off[i][1], R.flip_bits(D[i], i % 40))
    exp_moved = np.concatenate([_obs(pos[i][0] + 16, pos[i][1] - 8, 63 - i, i % 40, -1, ALL) if i < 64 else
                                _obs(pos[i][0] + 16, pos[i][1] - 8) for i in range(130)])

    frames = [_finish(full, lms, exp_full, poison=poison), _finish(empty, lms, exp_empty, poison=poison),
              _finish(some, lms, exp_some, poison=poison), _finish(moved, lms, exp_moved, poison=poison)]
    # ranges that overlap: the second half of the grid, in the full frame
    tail = _finish(full, lms, exp_full[65:], poison=poison)
    tail["name"], tail["sub"] = "grid tail (overlapping range)", (65, 65)
    return lms, frames + [tail]


def _window_and_borders(rng):
    D = R.random_descriptors(rng, 16)
    f = _Frame("window edges and image borders")
    lms, exp = [], []
    up, down = np.nextafter(np.float32(215), np.float32(1e9)), np.nextafter(np.float32(165), np.float32(0))
    # |dx| == r is inside, the next float outside; likewise |dy|
    lms.append(R.make_landmark(100, 100, D[0])); exp.append(_obs(100, 100, f.add(115, 100, R.flip_bits(D[0], 5)), 5, -1, ALL))
    lms.append(R.make_landmark(200, 100, D[1])); f.add(up, 100, D[1]); exp.append(_obs(200, 100))
    lms.append(R.make_landmark(100, 180, D[2])); exp.append(_obs(100, 180, f.add(100, 165, D[2]), 0, -1, ALL))
    lms.append(R.make_landmark(200, 180, D[3])); f.add(200, down, D[3]); exp.append(_obs(200, 180))
    # u = width and v = height are outside, u = 0 and v = 0 inside, u = -1 outside
    lms.append(R.make_landmark(320, 40, D[4])); f.add(319, 40, D[4]); exp.append(_hidden())
    lms.append(R.make_landmark(0, 40, D[5])); exp.append(_obs(0, 40, f.add(3, 40, D[5]), 0, -1, ALL))
    lms.append(R.make_landmark(40, 240, D[6])); f.add(40, 239, D[6]); exp.append(_hidden())
    lms.append(R.make_landmark(280, 0, D[7])); exp.append(_obs(280, 0, f.add(280, 2, D[7]), 0, -1, ALL))
    lms.append(R.make_landmark(-1, 140, D[8])); f.add(1, 140, D[8]); exp.append(_hidden())
    # a keypoint OUTSIDE the image is a candidate all the same: the rules test the window alone
    lms.append(R.make_landmark(2, 220, D[9])); exp.append(_obs(2, 220, f.add(-4, 221, R.flip_bits(D[9], 2)), 2, -1, ALL))
    return np.concatenate(lms), [_finish(f, np.concatenate(lms), np.concatenate(exp))]


def _depth_and_dead(rng):
    D = R.random_descriptors(rng, 1)[0]
    f = _Frame("depth, dead landmarks, NaN and Inf")
    k = f.add(160, 120, D)                                                     # a perfect match for whoever is visible at the centre
    lms = [R.make_landmark(160, 120, D, z=0.1),                               # Xc.z == min_depth: out
           R.make_landmark(160, 120, D, z=np.nextafter(0.1, 1.0)),            # the next double: in, X = (0, 0, z) projects to (cx, cy)
           R.make_landmark(160, 120, D, z=-4.0),                              # behind the camera
           R.make_landmark(160, 120, D, octave=-1),                           # dead
           R.make_landmark(160, 120, D), R.make_landmark(160, 120, D), R.make_landmark(160, 120, D), R.make_landmark(160, 120, D)]
    lms[4]["X"][0, 0] = np.nan
    lms[5]["X"][0, 2] = np.nan
    lms[6]["X"][0, 1] = np.inf
    lms[7]["X"][0, 0] = 1e300                                                  # finite in fp64, Inf as fp32 pixel
    exp = [_hidden(), _obs(160, 120, k, 0, -1, ALL)] + [_hidden()] * 6
    return np.concatenate(lms), [_finish(f, np.concatenate(lms), np.concatenate(exp))]


def _ties_and_thresholds(rng):
    D = R.random_descriptors(rng, 8)
    f = _Frame("ties, single candidates, thresholds")
    lms, exp = [], []
    # two candidates at equal distance: the lowest k is the best, second == hamming, the ratio rejects
    lms.append(R.make_landmark(40, 40, D[0]))
    f.add(42, 40, R.flip_bits(D[0], 7)); f.add(38, 40, R.flip_bits(D[0], 7, start=100))
    exp.append(_obs(40, 40, -1, 7, 7, R.VISIBLE | R.CANDIDATES))
    # a single candidate passes the ratio test, at th_hamming - 1
    lms.append(R.make_landmark(100, 40, D[1])); exp.append(_obs(100, 40, f.add(100, 41, R.flip_bits(D[1], 99)), 99, -1, ALL))
    # hamming == th_hamming is rejected
    lms.append(R.make_landmark(160, 40, D[2])); f.add(160, 41, R.flip_bits(D[2], 100)); exp.append(_obs(160, 40, -1, 100, -1, 3))
    # the ratio in fp32: 0.9f * 10.0f rounds to 9.0f, so 9 against 10 is rejected and 8 against 10 accepted
    lms.append(R.make_landmark(220, 40, D[3]))
    f.add(221, 40, R.flip_bits(D[3], 10)); f.add(219, 40, R.flip_bits(D[3], 9, start=50))
    exp.append(_obs(220, 40, -1, 9, 10, 3))
    lms.append(R.make_landmark(280, 40, D[4]))
    f.add(281, 40, R.flip_bits(D[4], 10))
    k = f.add(279, 40, R.flip_bits(D[4], 8, start=50))
    exp.append(_obs(280, 40, k, 8, 10, ALL))
    # the runner-up may come first in k: best is still the least distance
    lms.append(R.make_landmark(40, 120, D[5]))
    f.add(41, 120, R.flip_bits(D[5], 80)); f.add(41, 121, R.flip_bits(D[5], 70))
    k = f.add(39, 120, R.flip_bits(D[5], 1))
    exp.append(_obs(40, 120, k, 1, 70, ALL))
    return np.concatenate(lms), [_finish(f, np.concatenate(lms), np.concatenate(exp))]


def _uniqueness(rng):
    D = R.random_descriptors(rng, 4)
    f = _Frame("two landmarks claim one keypoint")
    # equal distance (6 and 6): the lower i wins, the loser keeps bits 0-2
    da, db = D[0], R.flip_bits(D[0], 12)
    k0 = f.add(102, 100, R.flip_bits(da, 6))
    # unequal distance (9 and 5): the lesser wins although its i is higher
    kd = R.flip_bits(D[1], 9)
    k1 = f.add(202, 100, kd)
    dd = R.flip_bits(kd, 5, start=100)
    lms = [R.make_landmark(100, 100, da), R.make_landmark(104, 100, db), R.make_landmark(200, 100, D[1]), R.make_landmark(204, 100, dd)]
    exp = [_obs(100, 100, k0, 6, -1, ALL), _obs(104, 100, -1, 6, -1, 7), _obs(200, 100, -1, 9, -1, 7), _obs(204, 100, k1, 5, -1, ALL)]
    return np.concatenate(lms), [_finish(f, np.concatenate(lms), np.concatenate(exp))]


def _octaves(rng):
    D = R.random_descriptors(rng, 3)
    f = _Frame("octave differences and clamping")
    # octave 2 (r = 21.6): a difference of 1 is a candidate, of 2 is not -- even at distance 0 on the projection itself
    ka = f.add(118, 30, R.flip_bits(D[0], 10), octave=3)                       # |dx| = 18 > 15: inside only because r grows with the octave
    f.add(100, 30, D[0], octave=4)
    # octave 9 clamps to 7 (r = 53.7): octave 6 and octave 9 (-> 7) are candidates, octave 5 is not
    kb = f.add(200, 170, R.flip_bits(D[1], 3), octave=6)
    f.add(250, 120, R.flip_bits(D[1], 20), octave=9)
    f.add(200, 120, D[1], octave=5)
    # a negative keypoint octave clamps to 0
    kc = f.add(60, 200, R.flip_bits(D[2], 2), octave=-3)
    lms = [R.make_landmark(100, 30, D[0], octave=2), R.make_landmark(200, 120, D[1], octave=9), R.make_landmark(60, 210, D[2], octave=1)]
    exp = [_obs(100, 30, ka, 10, -1, ALL), _obs(200, 120, kb, 3, 20, ALL), _obs(60, 210, kc, 2, -1, ALL)]
    return np.concatenate(lms), [_finish(f, np.concatenate(lms), np.concatenate(exp))]


def _repeated_texture(rng):
    """Six pairs of landmarks with IDENTICAL descriptors, the two of a pair 80 px apart (more than 2 r), and a keypoint on each
    with the same three bits flipped. Brute force with a ratio test sees two equal best distances for every landmark and keeps
    none; the window tells them apart."""
    D = R.random_descriptors(rng, 6)
    f = _Frame("repeated texture")
    lms, exp = [], []
    for row in range(2):
        for p in range(6):
            u, v = 40 + 40 * p, 60 + 80 * row
            lms.append(R.make_landmark(u, v, D[p]))
            exp.append(_obs(u, v, f.add(u + 1, v + 1, R.flip_bits(D[p], 3)), 3, -1, ALL))
    return np.concatenate(lms), [_finish(f, np.concatenate(lms), np.concatenate(exp))]


def _one_and_a_chunk(rng):
    """CHUNK + 1 landmarks 16 px apart (more than r): a keypoint ON landmarks 0, CHUNK - 1 and CHUNK is a candidate of that one
    alone."""
    n = CHUNK + 1
    pos = [(10 + 16 * (i % 19), 10 + 16 * (i // 19)) for i in range(n)]
    D = R.random_descriptors(rng, n)
    lms = np.concatenate([R.make_landmark(u, v, D[i]) for i, (u, v) in enumerate(pos)])
    f = _Frame("a range of one chunk + 1")
    hit = {i: f.add(pos[i][0], pos[i][1], D[i]) for i in (CHUNK, 0, CHUNK - 1)}
    exp = np.concatenate([_obs(pos[i][0], pos[i][1], hit[i], 0, -1, ALL) if i in hit else _obs(*pos[i]) for i in range(n)])
    return lms, [_finish(f, lms, exp)]


@functools.lru_cache(maxsize=None)
def table():
    """dict(landmarks, frames, ...). A frame: name, pose (12), kp / desc (the n real ones), n (what d_n says), first, count, valid,
    exp (the written-down records of its range; None when invalid), poison (keypoints + descriptors for the slots beyond n)."""
    rng = np.random.default_rng(2024)
    landmarks, frames = [], []
    at = 0
    for group in (_grid, _window_and_borders, _depth_and_dead, _ties_and_thresholds, _uniqueness, _octaves, _repeated_texture,
                  _one_and_a_chunk):
        lms, fs = group(rng)
        for f in fs:
            off, cnt = f.pop("sub", (0, len(lms)))
            f["first"], f["count"] = at + off, cnt
            frames.append(f)
        landmarks.append(lms)
        at += len(lms)
    landmarks = np.concatenate(landmarks)
    grid_full = frames[0]
    # count 0 in the middle of the array: nothing is visible, nothing read
    zero = dict(grid_full, name="count 0", first=7, count=0, exp=R.not_visible_obs(0))
    frames.insert(3, zero)
    # every way a frame can be invalid, between valid neighbours; their keypoint slots hold only poison
    nan_pose, inf_pose = R.IDENTITY_POSE.copy(), R.IDENTITY_POSE.copy()
    nan_pose[5], inf_pose[11] = np.nan, -np.inf
    bad = [("n < 0", dict(n=-1)), ("n > kp_stride", dict(n=KP_STRIDE + 1)), ("first < 0", dict(first=-1)),
           ("count < 0", dict(count=-1)), ("count > land_cap", dict(count=LAND_CAP + 1)),
           ("first + count > n_landmarks", dict(first=len(landmarks) - 129)), ("NaN in the pose", dict(pose=nan_pose)),
           ("Inf in the pose", dict(pose=inf_pose))]
    for j, (name, change) in enumerate(bad):
        f = dict(grid_full, name="invalid: " + name, valid=False, exp=None, **change)
        frames.insert(1 + 2 * j, f)
    for f in frames:
        assert f["kp"].dtype == KP_DTYPE and len(f["kp"]) <= KP_STRIDE and (f["exp"] is None or len(f["exp"]) == f["count"] <= LAND_CAP)
    return dict(landmarks=landmarks, frames=frames, cfg=CFG, width=W, height=H, kp_stride=KP_STRIDE, land_cap=LAND_CAP)


def frame_arrays(f):
    """The frame's kp_stride keypoint and descriptor slots: the real ones, then poison."""
    kp = np.zeros(KP_STRIDE, KP_DTYPE)
    desc = np.zeros((KP_STRIDE, 32), np.uint8)
    pk, pd = f["poison"] if f["poison"] is not None else (R.make_keypoint(160, 120), np.zeros((1, 32), np.uint8))
    for j in range(KP_STRIDE):
        kp[j], desc[j] = pk[j % len(pk)], pd[j % len(pd)]
    n = len(f["kp"]) if f["valid"] else 0
    kp[:n], desc[:n] = f["kp"][:n], f["desc"][:n]
    return kp, desc


def expected(f, landmarks):
    """(obs: LAND_CAP records, corr, pairs) of a frame from its written-down records and the output rule alone."""
    obs = R.not_visible_obs(LAND_CAP)
    if not f["valid"]:
        return obs, np.zeros(0, PNP_CORR_DTYPE), np.zeros(0, PROJ_PAIR_DTYPE)
    obs[:f["count"]] = f["exp"]
    won = np.flatnonzero(obs["flags"] & R.WON)
    corr, pairs = np.zeros(len(won), PNP_CORR_DTYPE), np.zeros(len(won), PROJ_PAIR_DTYPE)
    lm = landmarks.view(PROJ_LANDMARK_DTYPE)
    for j, i in enumerate(won):
        k = obs["kp_idx"][i]
        corr[j]["X"] = lm["X"][f["first"] + i]
        corr[j]["u"], corr[j]["v"] = f["kp"]["x"][k], f["kp"]["y"][k]
        pairs[j] = (f["first"] + i, k)
    return obs, corr, pairs


# ==== the second table: every limit and size the C-ABI admits ==============================================================
# table() above runs one configuration at one size. edge_groups() below is a list of groups, each ONE batch with its own
# configuration, image size, kp_stride and land_cap, so each runs on a handle of its own. Wherever a group says written=True
# its expected records are written down from the construction alone, as above; the restatement is run beside them, never
# in their place.
E20, E30 = 2.0 ** -20, 2.0 ** -30
COMPACT_ABOVE = 4096                                      # ranges longer than this go to the restatement as their live landmarks
_f32 = np.float32


def _landmark(K, u, v, desc, octave=0, z=R.EXACT_Z):
    """R.make_landmark for other principal points: with fx = fy = 256 and z = 4 every product and quotient of the projection
    is a dyadic rational far inside fp64, so a pixel that fp32 holds projects onto itself."""
    assert K[0] == K[1] == 256.0
    lm = np.zeros(1, PROJ_LANDMARK_DTYPE)
    lm["X"][0] = ((u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z)
    lm["desc"][0] = desc
    lm["octave"] = octave
    return lm


def _family(rng, m=6):
    """m descriptors 80 bits from one another (40 flipped bits each, disjoint), bits 240 .. 255 free for a keypoint's own
    noise: a landmark of member i is e bits from a keypoint of member i with e noise bits, and 80 + e from one of member j."""
    base = R.random_descriptors(rng, 1)[0]
    return [R.flip_bits(base, 40, start=40 * j) for j in range(m)]


def _noise(desc, e):
    return R.flip_bits(desc, e, start=240)


def _eframe(frame, exp, first=0, count=None, n=None, valid=True):
    kp = np.concatenate(frame.kp) if frame.kp else np.zeros(0, KP_DTYPE)
    desc = np.concatenate(frame.desc) if frame.desc else np.zeros((0, 32), np.uint8)
    return dict(name=frame.name, pose=frame.pose, kp=kp, desc=desc, n=len(kp) if n is None else n, first=first, count=count,
                valid=valid, exp=exp)


def _egroup(name, landmarks, frames, width=W, height=H, kp_stride=None, land_cap=None, written=True, **cfg):
    for f in frames:
        if f["count"] is None:
            f["count"] = len(landmarks)
        if f["exp"] is not None and not isinstance(f["exp"], np.ndarray):
            f["exp"] = np.concatenate(f["exp"])
        assert f["exp"] is None or len(f["exp"]) == f["count"]
    kp_stride = kp_stride or max(max(len(f["kp"]) for f in frames) + 3, 1)
    return dict(name=name, landmarks=landmarks, frames=frames, cfg=dict(dict(K=R.EXACT_K), **cfg), width=width, height=height,
                kp_stride=kp_stride, land_cap=land_cap or len(landmarks) + 2, written=written)


def _flip_rows(desc, nbits, start):
    """flip_bits for many rows at once: row j is desc with nbits[j] bits flipped from bit start[j] on."""
    bits = np.tile(np.unpackbits(np.asarray(desc, np.uint8), bitorder="little"), (len(nbits), 1))
    b = np.arange(256)[None, :]
    bits ^= ((b >= start[:, None]) & (b < (start + nbits)[:, None])).astype(np.uint8)
    return np.packbits(bits, axis=1, bitorder="little")


# ---- index_bits: the 13-bit index field of the running top-2 ---------------------------------------------------------------
def _index_bits(rng):
    """n = kp_stride = 8192. 8186 keypoints are parked on the row y = 236, which no window reaches (the lowest ends at 75).
    Contest 1 (L0): k = 8191 at distance 3, k = 5 at 4, k = 9 at 5: best 8191, second 4. Contest 2 (L1): k = 4095 and k = 4096
    at distance 7 each: the lower k is the best, second == hamming, the ratio rejects (a key whose index field is 12 bits
    wide reads 4096 as one more bit of distance and accepts). L2 has k = 8191 as its single candidate, at distance 5; L3 has
    k = 7 at distance 1 as best and k = 8191 at distance 20 as SECOND. Frame A searches all four: L0 and L2 both claim 8191
    (contest 4), L0 wins by distance. Frame B searches L1 .. L3: L2 wins 8191 as a single candidate (contest 3)."""
    N = 8192
    D = R.random_descriptors(rng, 4)
    kp = np.zeros(N, KP_DTYPE)
    kp["x"], kp["y"] = 2 + (np.arange(N) % 310), 236
    kp["size"], kp["response"] = 31.0, 1.0
    desc = R.random_descriptors(rng, N)
    e = R.flip_bits(D[0], 3)                                                   # the descriptor of keypoint 8191
    d3 = R.flip_bits(e, 20, start=128)                                         # L3: 20 bits from keypoint 8191
    put = {8191: (50, 40, e), 5: (30, 40, R.flip_bits(D[0], 4, start=50)), 9: (28, 42, R.flip_bits(D[0], 5, start=100)),
           4095: (101, 40, R.flip_bits(D[1], 7)), 4096: (99, 40, R.flip_bits(D[1], 7, start=100)), 7: (62, 60, R.flip_bits(d3, 1))}
    for k, (x, y, d) in put.items():
        kp["x"][k], kp["y"][k], desc[k] = x, y, d
    lms = np.concatenate([R.make_landmark(40, 40, D[0]), R.make_landmark(100, 40, D[1]),
                          R.make_landmark(64, 40, R.flip_bits(e, 5, start=200)), R.make_landmark(60, 50, d3)])
    a, b = _Frame("index_bits A: all four"), _Frame("index_bits B: the single candidate wins")
    for f in (a, b):
        f.kp, f.desc = [kp], [desc]
    exp_a = [_obs(40, 40, 8191, 3, 4, ALL), _obs(100, 40, -1, 7, 7, 3), _obs(64, 40, -1, 5, -1, 7), _obs(60, 50, 7, 1, 20, ALL)]
    exp_b = [_obs(100, 40, -1, 7, 7, 3), _obs(64, 40, 8191, 5, -1, ALL), _obs(60, 50, 7, 1, 20, ALL)]
    return _egroup("index_bits", lms, [_eframe(a, exp_a), _eframe(b, exp_b, first=1, count=3)], kp_stride=N, land_cap=6)


# ---- claim_bits: the 20-bit landmark field of the claim key -----------------------------------------------------------------
CLAIM_LIVE = (0, 3, 4095, 4096, 65535, 65536, 65541, 1 << 19, (1 << 19) + 7, (1 << 20) - 1)


def _claim_bits(rng):
    """land_cap = count = 2^20, every landmark dead except CLAIM_LIVE. The dead ones all sit ON keypoint 0 with its
    descriptor, so a dead landmark read as live shows. The keypoints of the layouts are 60 px apart, a landmark is within
    2 px of its own, so each has one candidate and every claim is decided by the key alone:
      a  keypoint 0: i = 2^20 - 1 at Hamming 4 against i = 0 at 5: the higher i wins by distance.
      b  keypoint 1: i = 65541 at 5 against i = 3 at 6: 65541 wins (a shift of 16 lets i reach into the distance: 3 wins).
      c  keypoint 2: i = 65535 and i = 65536 at 2 each: 65535 wins (i cut to 16 bits: 65536 reads as 0 and wins).
      d  keypoint 3: i = 2^19 alone at 1 (i cut to 19 bits on the claiming side alone: its word never holds its key).
      e  keypoint 4: i = 4096 and i = 2^19 + 7 at 4 each, i = 4095 at 5: 4096 wins. 2^19 + 7 is not on the issue's list: it is
         here because an i cut to 19 bits on BOTH sides of the claim is invisible to a - d (2^19 + 7 reads as 7 and wins).
    Twenty more keypoints lie on the rows y = 200 and y = 220, which no window reaches."""
    NL = 1 << 20
    D = R.random_descriptors(rng, 5)
    f = _Frame("claim_bits")
    centres = [(40, 40), (100, 40), (160, 40), (220, 40), (40, 120)]
    for (x, y), d in zip(centres, D):
        f.add(x, y, d)
    far = R.random_descriptors(rng, 20)
    for j in range(20):
        f.add(10 + 15 * (j % 10), 200 + 20 * (j // 10), far[j])
    lms = np.zeros(NL, PROJ_LANDMARK_DTYPE)
    lms["X"], lms["desc"], lms["octave"], lms["source"] = R.exact_point(40, 40), D[0], -1, np.arange(NL)
    exp = R.not_visible_obs(NL)
    #        i            keypoint  du  bits  start  won
    live = [(NL - 1,          0,     1,  4,    0,   True), (0, 0, -1, 5, 64, False),
            (65541,           1,     1,  5,    0,   True), (3, 1, -1, 6, 64, False),
            (65535,           2,     1,  2,    0,   True), (65536, 2, -1, 2, 64, False),
            (1 << 19,         3,     2,  1,    0,   True),
            (4096,            4,     1,  4,    0,   True), ((1 << 19) + 7, 4, -1, 4, 64, False), (4095, 4, 2, 5, 128, False)]
    assert sorted(r[0] for r in live) == list(CLAIM_LIVE)
    for i, k, du, bits, start, won in live:
        u, v = centres[k][0] + du, centres[k][1]
        lm = R.make_landmark(u, v, R.flip_bits(D[k], bits, start=start), source=i)
        lms[i] = lm[0]
        exp[i] = _obs(u, v, k if won else -1, bits, -1, ALL if won else 7)[0]
    return _egroup("claim_bits", lms, [_eframe(f, exp)], kp_stride=32, land_cap=NL)


# ---- grids: one cell, one row, one column, two cells and 16384 cells --------------------------------------------------------
def _site(K, f, lms, exp, desc, p, axis, side, dist, other=None):
    """A keypoint at p, `dist` bits from desc. Landmark A lies 15 px from it along `axis` (on the `side` given), so the keypoint
    is ON the edge of A's window: a candidate. Landmark B's coordinate is the NEXT fp32 beyond A's: its window stops one float
    short. `other`: the landmarks' coordinate on the other axis when it is not the keypoint's."""
    k = f.add(p[0], p[1], R.flip_bits(desc, dist))
    c = _f32(p[axis])
    ca = _f32(c + _f32(side * 15))
    cb = np.nextafter(ca, _f32(side * 1e9))
    assert float(ca) == p[axis] + side * 15 and abs(c - ca) == _f32(15) and abs(c - cb) > _f32(15)   # the fp32 differences of rule 2
    for cc, hit in ((ca, True), (cb, False)):
        q = [p[0], p[1]] if other is None else ([0, other] if axis == 0 else [other, 0])
        q[axis] = float(cc)
        lms.append(_landmark(K, q[0], q[1], desc))
        exp.append(_obs(q[0], q[1], k, dist, -1, ALL) if hit else _obs(q[0], q[1]))


GRID_K = (256.0, 256.0, 16.0, 16.0)     # every grid: u = 256 x / 4 + 16 is exact for x = (u - 16) / 64, so one handle serves all five sizes


def _grid_full(rng):
    """4096 x 4096, K = GRID_K: 128 x 128 = 16384 cells, 65 KiB of dynamic LDS in k_proj_bin. A keypoint in
    each corner cell ((0, 0), (127, 0), (0, 127), (127, 127)), in the interior cell (64, 37) and 2 - 3 px outside each image
    edge, each with the two landmarks of _site; and a landmark of octave 2 with a keypoint 18 px away: inside only because
    the radius grows with the level."""
    K = GRID_K
    D = R.random_descriptors(rng, 10)
    f = _Frame("grid 4096x4096")
    lms, exp = [], []
    sites = [((3, 5), 0, 1), ((4090, 4), 0, -1), ((6, 4091), 1, -1), ((4092, 4093), 1, -1), ((2053, 1193), 0, 1),
             ((-3, 1000), 0, 1), ((4098, 1200), 0, -1), ((1000, -2), 1, 1), ((1300, 4097.5), 1, -1)]
    for j, (p, axis, side) in enumerate(sites):
        _site(K, f, lms, exp, D[j], p, axis, side, j)
    lms.append(_landmark(K, 3000, 3000, D[9], octave=2))
    exp.append(_obs(3000, 3000, f.add(3018, 3000, R.flip_bits(D[9], 3), octave=2), 3, -1, ALL))
    return _egroup("grid 4096x4096", np.concatenate(lms), [_eframe(f, exp)], width=4096, height=4096, K=K)


def _grid_strip(rng, horizontal):
    """4096 x 1 (128 cells in one row) and its transpose 1 x 4096 (one column), K = GRID_K. Every landmark has 0.5 on the short
    axis. Keypoints in the first cell (31), the last (4064) and a middle one and beyond both ends (-3, 4098), two of them 10.5
    and 11.5 px off the strip: outside the image and inside the window. The windows of 31 and -3, of 4064 and 4098 are
    disjoint."""
    name = "4096x1" if horizontal else "1x4096"
    K = GRID_K
    D = R.random_descriptors(rng, 5)
    f = _Frame("grid " + name)
    lms, exp = [], []
    axis = 0 if horizontal else 1
    for j, (c, o, side) in enumerate([(31, 0.5, 1), (4064, 0.25, -1), (2053, -10, 1), (-3, 12, 1), (4098, 0.5, -1)]):
        _site(K, f, lms, exp, D[j], (c, o) if horizontal else (o, c), axis, side, j + 1, other=0.5)
    w, h = (4096, 1) if horizontal else (1, 4096)
    return _egroup("grid " + name, np.concatenate(lms), [_eframe(f, exp)], width=w, height=h, K=K)


def _grid_one_cell(rng):
    """32 x 32, K = GRID_K: one cell. A window of 15 px covers most of the image, so landmarks share keypoints;
    descriptors come from one family, which makes every distance known: e to the own keypoint, 80 + e to another's."""
    K = GRID_K
    D = _family(rng)
    f = _Frame("grid 32x32")
    k = [f.add(2, 2, _noise(D[0], 1)), f.add(30, 30, _noise(D[1], 2)), f.add(-5, 16, _noise(D[2], 3)), f.add(16, 40, _noise(D[3], 4))]
    lms = [_landmark(K, 16, 16, D[0]),       # window [1, 31]^2: k0 (1) and k1 (82)
           _landmark(K, 20, 25, D[1]),       # [5, 35] x [10, 40]: k1 (2) and k3 on the edge dy == 15 (84)
           _landmark(K, 0, 16, D[2]),        # [-15, 15] x [1, 31]: k0 (81) and k2 outside the image (3)
           _landmark(K, 16, 31.5, D[3]),     # [1, 31] x [16.5, 46.5]: k1 (82) and k3 outside the image (4)
           _landmark(K, 31, 0, D[4]),        # [16, 46] x [-15, 15]: nobody
           _landmark(K, 32, 5, D[0]), _landmark(K, 5, 32, D[0])]               # u == width, v == height
    exp = [_obs(16, 16, k[0], 1, 82, ALL), _obs(20, 25, k[1], 2, 84, ALL), _obs(0, 16, k[2], 3, 81, ALL), _obs(16, 31.5, k[3], 4, 82, ALL),
           _obs(31, 0), _hidden(), _hidden()]
    return _egroup("grid 32x32", np.concatenate(lms), [_eframe(f, exp)], width=32, height=32, K=K)


def _grid_two_cells(rng):
    """33 x 31, K = GRID_K: two cells in x, one in y. k0 at x = 31.5 is in cell 0, k1 at 32.5 and k2 at 40 (outside
    the image) in cell 1."""
    K = GRID_K
    D = _family(rng)
    f = _Frame("grid 33x31")
    k = [f.add(31.5, 10, _noise(D[0], 1)), f.add(32.5, 20, _noise(D[1], 2)), f.add(40, 30, _noise(D[2], 3))]
    lms = [_landmark(K, 32, 5, D[0]),        # [17, 47] x [-10, 20]: k0 (1), k1 on the edge dy == 15 (82)
           _landmark(K, 20, 30, D[1]),       # [5, 35] x [15, 45]: k1 (2)
           _landmark(K, 32.5, 30.5, D[2]),   # [17.5, 47.5] x [15.5, 45.5]: k1 (82), k2 (3)
           _landmark(K, 33, 10, D[0]), _landmark(K, 10, 31, D[0]),             # u == width, v == height
           _landmark(K, 0, 0, D[3])]         # [-15, 15]^2: nobody
    exp = [_obs(32, 5, k[0], 1, 82, ALL), _obs(20, 30, k[1], 2, -1, ALL), _obs(32.5, 30.5, k[2], 3, 82, ALL), _hidden(), _hidden(), _obs(0, 0)]
    return _egroup("grid 33x31", np.concatenate(lms), [_eframe(f, exp)], width=33, height=31, K=K)


# ---- spans: a cell of 8192 keypoints, and windows that cover the whole grid ---------------------------------------------------
SPAN_BEST, SPAN_SECOND = 5003, 7010


def _span_one_cell(rng):
    """n = kp_stride = 8192, all in cell (1, 1) on the pixels x = 33 + k % 30, y = 33 + (k // 30) % 30, all inside the window of
    the landmark at (48, 48): one span of 8192 entries, 512 steps of the 16-lane walk. Every keypoint is 60 + k % 7 bits from
    the landmark except k = 5003 (2 bits) and k = 7010 (9 bits): in k order, which the scatter follows up to the order of its
    atomics, lanes 11 and 2, both far past the 32nd entry. A second landmark at (200, 200) sees nothing."""
    N = 8192
    D = R.random_descriptors(rng, 1)[0]
    k = np.arange(N)
    kp = np.zeros(N, KP_DTYPE)
    kp["x"], kp["y"] = 33 + k % 30, 33 + (k // 30) % 30
    kp["size"], kp["response"] = 31.0, 1.0
    desc = _flip_rows(D, 60 + k % 7, (k * 13) % 190)
    desc[SPAN_BEST], desc[SPAN_SECOND] = R.flip_bits(D, 2), R.flip_bits(D, 9, start=30)
    assert SPAN_BEST % 16 != SPAN_SECOND % 16 and min(SPAN_BEST, SPAN_SECOND) > 32
    f = _Frame("span of 8192 in one cell")
    f.kp, f.desc = [kp], [desc]
    lms = np.concatenate([R.make_landmark(48, 48, D), R.make_landmark(200, 200, D)])
    return _egroup("spans one cell", lms, [_eframe(f, [_obs(48, 48, SPAN_BEST, 2, 9, ALL), _obs(200, 200)])], kp_stride=N, land_cap=3)


BAD_COORDS = (np.nan, np.inf, -np.inf, 3e38, -3e38)


def _span_whole_grid(rng):
    """radius_px = 1024 on 320 x 240: every window is the whole grid of 80 cells. k0 at x = -1000 and k1 at y = 1200 are far
    outside the image and inside a window; seven keypoints at +-3e38, +-Inf and NaN carry perfect matches and are never
    candidates. One descriptor family, so: L0 (20, 120) has k0 alone (|dy| to k1 is 1080); L1 (100, 200) has k1 alone (|dx| to
    k0 is 1100); L2 (10, 180) has both, 81 against 82, and the ratio rejects."""
    D = _family(rng)
    f = _Frame("windows of the whole grid")
    k0, k1 = f.add(-1000, 100, _noise(D[0], 1)), f.add(100, 1200, _noise(D[1], 2))
    for j, (x, y) in enumerate([(3e38, 120), (-3e38, 120), (100, np.inf), (100, -np.inf), (np.nan, 120), (100, np.nan), (np.nan, np.nan)]):
        f.add(x, y, D[j % 3])
    lms = np.concatenate([R.make_landmark(20, 120, D[0]), R.make_landmark(100, 200, D[1]), R.make_landmark(10, 180, D[2])])
    exp = [_obs(20, 120, k0, 1, -1, ALL), _obs(100, 200, k1, 2, -1, ALL), _obs(10, 180, -1, 81, 82, 3)]
    return _egroup("spans whole grid", lms, [_eframe(f, exp)], radius_px=1024.0)


def _span_whole_big_grid(rng):
    """radius_px = 1024 on 4096 x 4096, K = GRID_K: a landmark of octave 7 at the centre has r = 1024 * 1.2^7 = 3669 px, so its
    window is all 16384 cells, 128 rows of 128. Its candidates (octave 6 or 7): k0 in the first cell (1 bit), k1 in the last
    (octave 6, 82), k3 at (-1000, 5000), outside the image (83). k2 (octave 5, a perfect match) fails the octave test and k4
    (x = -2000, a perfect match) the window: |dx| = 4048. A landmark of octave 0 at (100, 100) has k5 (octave 1) alone."""
    D = _family(rng)
    f = _Frame("a window of 16384 cells")
    k0 = f.add(3, 5, _noise(D[0], 1), octave=7)
    f.add(4090, 4093, _noise(D[1], 2), octave=6)
    f.add(2000, 100, D[0], octave=5)
    f.add(-1000, 5000, _noise(D[2], 3), octave=7)
    f.add(-2000, 2048, D[0], octave=7)
    k5 = f.add(1100, 1100, _noise(D[3], 4), octave=1)
    assert 3660 < 1024 * R.level_scales()[7] < 4048
    lms = np.concatenate([_landmark(GRID_K, 2048, 2048, D[0], octave=7), _landmark(GRID_K, 100, 100, D[3])])
    exp = [_obs(2048, 2048, k0, 1, 82, ALL), _obs(100, 100, k5, 4, -1, ALL)]
    return _egroup("spans whole 4096 grid", lms, [_eframe(f, exp)], width=4096, height=4096, K=GRID_K, radius_px=1024.0)


# ---- limits: one scene under configurations that differ from the defaults in one field, set to an end of its range ----------
LIMIT_CONFIGS = {"defaults": {}, "radius_px=0": dict(radius_px=0.0), "ratio=0": dict(ratio=0.0), "ratio=1": dict(ratio=1.0),
                 "th_hamming=0": dict(th_hamming=0), "th_hamming=257": dict(th_hamming=257), "max_octave_diff=0": dict(max_octave_diff=0),
                 "max_octave_diff=8": dict(max_octave_diff=8), "min_depth=-1": dict(min_depth=-1.0)}


def _limits(rng, which):
    """Fifteen landmarks, each at least 60 px from the next group, so a keypoint is a candidate of its own landmarks alone.
    Each row of `rec` is a landmark: its record under the defaults, then the configurations under which it differs."""
    D = R.random_descriptors(rng, 16)
    f = _Frame("limits " + which)
    vis = lambda u, v: _obs(u, v)   # noqa: E731
    rec, lms = [], []

    def add(lm, default, **other):
        lms.append(lm)
        rec.append(other.get(which.replace("=", "_").replace("-", "m"), default))

    # S0 and S16 project onto the pixel of keypoint a0: a candidate even at radius 0; S16 loses the claim (5 against 3)
    da = R.flip_bits(D[0], 3)
    a0 = f.add(30, 30, da)
    add(R.make_landmark(30, 30, D[0]), _obs(30, 30, a0, 3, -1, ALL), th_hamming_0=_obs(30, 30, -1, 3, -1, 3))
    add(R.make_landmark(30, 30, R.flip_bits(da, 5, start=100)), _obs(30, 30, -1, 5, -1, 7), th_hamming_0=_obs(30, 30, -1, 5, -1, 3))
    # S1: a single candidate at distance 0, 5 px away: th_hamming = 0 rejects even that
    a1 = f.add(95, 30, D[1])
    add(R.make_landmark(90, 30, D[1]), _obs(90, 30, a1, 0, -1, ALL), radius_px_0=vis(90, 30), th_hamming_0=_obs(90, 30, -1, 0, -1, 3))
    # S2: 0 against 0: 0 < ratio * 0 holds for no ratio
    f.add(151, 30, D[2]); f.add(149, 30, D[2])
    add(R.make_landmark(150, 30, D[2]), _obs(150, 30, -1, 0, 0, 3), radius_px_0=vis(150, 30))
    # S3: 9 against 10: rejected at 0.9 (0.9f * 10.0f rounds to 9.0f), accepted at ratio 1
    f.add(211, 30, R.flip_bits(D[3], 10))
    c1 = f.add(209, 30, R.flip_bits(D[3], 9, start=50))
    add(R.make_landmark(210, 30, D[3]), _obs(210, 30, -1, 9, 10, 3), radius_px_0=vis(210, 30), ratio_1=_obs(210, 30, c1, 9, 10, ALL))
    # S4: 10 against 10: rejected at ratio 1 too
    f.add(271, 30, R.flip_bits(D[4], 10)); f.add(269, 30, R.flip_bits(D[4], 10, start=50))
    add(R.make_landmark(270, 30, D[4]), _obs(270, 30, -1, 10, 10, 3), radius_px_0=vis(270, 30))
    # S5: u = 0 and xk = -0.0: |xk - u| == 0 <= 0
    k5 = f.add(-0.0, 90, R.flip_bits(D[5], 2))
    assert np.signbit(f.kp[k5]["x"][0])
    add(R.make_landmark(0, 90, D[5]), _obs(0, 90, k5, 2, -1, ALL), th_hamming_0=_obs(0, 90, -1, 2, -1, 3))
    # S6: the complemented descriptor ON the projection: distance 256, accepted by th_hamming = 257 alone
    d0 = f.add(90, 90, ~D[6])
    add(R.make_landmark(90, 90, D[6]), _obs(90, 90, -1, 256, -1, 3), th_hamming_257=_obs(90, 90, d0, 256, -1, ALL))
    # S7 and S8 share keypoint d1: 256 against 255, the 255 takes it
    d1 = f.add(152, 90, ~D[7])
    add(R.make_landmark(150, 90, D[7]), _obs(150, 90, -1, 256, -1, 3), radius_px_0=vis(150, 90), th_hamming_257=_obs(150, 90, -1, 256, -1, 7))
    add(R.make_landmark(155, 90, R.flip_bits(~D[7], 255)), _obs(155, 90, -1, 255, -1, 3), radius_px_0=vis(155, 90),
        th_hamming_257=_obs(155, 90, d1, 255, -1, ALL))
    # S9 (octave 0): e0 octave 1 at 1 bit, e1 octave 7 at 0 bits, e2 octave 0 at 20 bits
    e0, e1, e2 = f.add(212, 90, R.flip_bits(D[9], 1), octave=1), f.add(208, 90, D[9], octave=7), f.add(210, 93, R.flip_bits(D[9], 20, start=60))
    add(R.make_landmark(210, 90, D[9]), _obs(210, 90, e0, 1, 20, ALL), radius_px_0=vis(210, 90), ratio_0=_obs(210, 90, -1, 1, 20, 3),
        th_hamming_0=_obs(210, 90, -1, 1, 20, 3), max_octave_diff_0=_obs(210, 90, e2, 20, -1, ALL), max_octave_diff_8=_obs(210, 90, e1, 0, 1, ALL))
    # S10, S11: z == 0 exactly passes min_depth = -1 and is hidden by its pixel: 0 / 0 is NaN, 64 / 0 is Inf
    for X in ((0.0, 0.0, 0.0), (0.25, 0.0, 0.0)):
        lm = R.make_landmark(160, 200, D[10])
        lm["X"][0] = X
        add(lm, _hidden())
    f.add(160, 200, D[10])
    # S12: z = -0.5 projects mirrored: u = -512 x + 160 = 270, v = -512 y + 120 = 90, exactly; visible under min_depth = -1 alone
    lm = R.make_landmark(270, 90, D[12])
    lm["X"][0] = (-0.21484375, 0.05859375, -0.5)
    f0 = f.add(270, 91, R.flip_bits(D[12], 4))
    add(lm, _hidden(), min_depth_m1=_obs(270, 90, f0, 4, -1, ALL))
    # S13: visible, no keypoint near
    add(R.make_landmark(30, 150, D[13]), vis(30, 150))
    return _egroup("limits " + which, np.concatenate(lms), [_eframe(f, rec)], **LIMIT_CONFIGS[which])


# ---- fp32: the window and the image test where fp32 and fp64 part ---------------------------------------------------------------
def _fp32(rng):
    """Default configuration, r = 15. With e = 2^-20 (the spacing of fp32 at 15):
      a  u = 0.75 e, xk = 15 + e: the real difference 15 + e / 4 exceeds r, the fp32 difference rounds to 15: a candidate.
      b  u = 0.25 e, xk = 15 + e: the fp32 difference is nextafter(15): not a candidate.
      c, d  the same pair in y.
      e  u = 320 - 2^-30 in fp64 is 320.0f: hidden.   f  v = 240 - 2^-30 likewise.   g  u = -2^-30 is negative in both: hidden.
    A perfect match waits near every hidden landmark and on b and d."""
    D = R.random_descriptors(rng, 7)
    f = _Frame("fp32")
    xk = _f32(15 + E20)
    ua, ub = _f32(0.75 * E20), _f32(0.25 * E20)
    assert float(xk) == 15 + E20 and float(ua) == 0.75 * E20 and float(ub) == 0.25 * E20          # all three are fp32 numbers
    assert float(xk) - float(ua) > 15 and xk - ua == _f32(15)                                      # a, c: fp64 says no, fp32 says yes
    assert xk - ub == np.nextafter(_f32(15), _f32(16))                                             # b, d
    assert 320 - E30 < 320 and _f32(320 - E30) == _f32(320) and 240 - E30 < 240 and _f32(240 - E30) == _f32(240)
    assert _f32(-E30) < 0
    lms = [R.make_landmark(0.75 * E20, 40, D[0]), R.make_landmark(0.25 * E20, 100, D[1]), R.make_landmark(100, 0.75 * E20, D[2]),
           R.make_landmark(200, 0.25 * E20, D[3]), R.make_landmark(320 - E30, 160, D[4]), R.make_landmark(60, 240 - E30, D[5]),
           R.make_landmark(-E30, 200, D[6])]
    for lm, (u, v) in zip(lms[:4], [(0.75 * E20, 40), (0.25 * E20, 100), (100, 0.75 * E20), (200, 0.25 * E20)]):
        X = lm["X"][0]                                                         # the projection is exact: no rounding before the cast
        assert 256.0 * X[0] / X[2] + 160.0 == u and 256.0 * X[1] / X[2] + 120.0 == v
    assert 256.0 * lms[4]["X"][0, 0] / 4.0 + 160.0 == 320 - E30 and 256.0 * lms[5]["X"][0, 1] / 4.0 + 120.0 == 240 - E30
    ka = f.add(xk, 40, R.flip_bits(D[0], 1))
    f.add(xk, 100, D[1])
    kc = f.add(100, xk, R.flip_bits(D[2], 2))
    f.add(200, xk, D[3])
    f.add(310, 160, D[4]); f.add(60, 235, D[5]); f.add(3, 200, D[6])
    exp = [_obs(ua, 40, ka, 1, -1, ALL), _obs(ub, 100), _obs(100, ua, kc, 2, -1, ALL), _obs(200, ub), _hidden(), _hidden(), _hidden()]
    return _egroup("fp32", np.concatenate(lms), [_eframe(f, exp)])


# ---- nonfinite_keypoints --------------------------------------------------------------------------------------------------------
def _bad_forms(x, y):
    """The fifteen keypoints that share a finite coordinate with (x, y) or none: NaN, +-Inf, +-3e38 in x, in y and in both."""
    return [(b, y) for b in BAD_COORDS] + [(x, b) for b in BAD_COORDS] + [(b, b) for b in BAD_COORDS]


def _nonfinite(rng):
    """320 x 240, 10 x 8 cells. Frame 1: an ordinary keypoint in cell 0 and one in the last cell, each 2 px from a landmark that
    must find it, among all fifteen non-finite forms of each, every one carrying the landmark's exact descriptor: k_proj_bin
    puts a NaN into cell 0 and an Inf or 3e38 into a border cell, and rule 2 refuses them all. Frame 2: a landmark and a keypoint
    on the centre of each of the other 30 border cells, and one non-finite form per landmark, cycling through the fifteen."""
    D = R.random_descriptors(rng, 32)
    f1, f2 = _Frame("non-finite keypoints around cell 0 and the last cell"), _Frame("non-finite keypoints around the other border cells")
    lms, exp1, exp2 = [], [], []
    for j, (u, v, xk) in enumerate([(10, 10, 12), (310, 230, 308)]):
        bad = _bad_forms(u, v)
        for x, y in bad[:8]:
            f1.add(x, y, D[j])
        k = f1.add(xk, v, R.flip_bits(D[j], j + 1))
        for x, y in bad[8:]:
            f1.add(x, y, D[j])
        lms.append(R.make_landmark(u, v, D[j]))
        exp1.append(_obs(u, v, k, j + 1, -1, ALL))
    border = [(cx, cy) for cy in range(8) for cx in range(10) if (cx in (0, 9) or cy in (0, 7)) and (cx, cy) not in ((0, 0), (9, 7))]
    assert len(border) == 30
    for j, (cx, cy) in enumerate(border):
        u, v = 32 * cx + 16, 32 * cy + 16 if cy < 7 else 32 * cy + 8           # the last row of cells is 16 px high
        x, y = _bad_forms(u, v)[j % 15]
        f2.add(x, y, D[2 + j])
        k = f2.add(u, v, R.flip_bits(D[2 + j], j % 5))
        lms.append(R.make_landmark(u, v, D[2 + j]))
        exp2.append(_obs(u, v, k, j % 5, -1, ALL))
    return _egroup("nonfinite_keypoints", np.concatenate(lms), [_eframe(f1, exp1, first=0, count=2), _eframe(f2, exp2, first=2, count=30)],
                   kp_stride=64)


@functools.lru_cache(maxsize=None)
def edge_groups():
    """The groups, in a fixed order. A group: name, cfg, width, height, kp_stride, land_cap, landmarks, written, frames; a frame:
    name, pose, kp / desc (the n real ones), n, first, count, valid, exp (the written records of its range)."""
    rng = np.random.default_rng(2025)
    groups = [_index_bits(rng), _claim_bits(rng), _grid_full(rng), _grid_strip(rng, True), _grid_strip(rng, False), _grid_one_cell(rng),
              _grid_two_cells(rng), _span_one_cell(rng), _span_whole_grid(rng)]
    groups += [_limits(np.random.default_rng(77), which) for which in LIMIT_CONFIGS]      # one scene: the same draws for each
    groups += [_fp32(rng), _nonfinite(rng), _span_whole_big_grid(rng)]
    for g in groups:
        for f in g["frames"]:
            assert f["kp"].dtype == KP_DTYPE and len(f["kp"]) <= g["kp_stride"] <= R.MAX_KP and f["count"] <= g["land_cap"] <= R.MAX_LAND
    assert len({g["name"] for g in groups}) == len(groups)
    return groups


def edge_group(name):
    return [g for g in edge_groups() if g["name"] == name][0]


def edge_frame_arrays(g, f):
    """The frame's kp_stride slots: the n real keypoints, then copies of them -- a slot beyond n read as a candidate is a
    duplicate at an equal distance, which changes `second`."""
    S, n = g["kp_stride"], len(f["kp"])
    kp, desc = np.zeros(S, KP_DTYPE), np.zeros((S, 32), np.uint8)
    kp[:n], desc[:n] = f["kp"], f["desc"]
    if n < S:
        j = np.arange(S - n) % max(n, 1)
        kp[n:], desc[n:] = (f["kp"][j], f["desc"][j]) if n else (R.make_keypoint(g["width"] / 2, g["height"] / 2), 0)
    return kp, desc


def edge_expected(g, f):
    """(obs: land_cap records, corr, pairs) of a frame from its written records and the output rule alone; no Python loop, the
    range may hold 2^20 records."""
    obs = R.not_visible_obs(g["land_cap"])
    obs[:f["count"]] = f["exp"]
    won = np.flatnonzero(obs["flags"] & R.WON)
    k = obs["kp_idx"][won]
    corr, pairs = np.zeros(len(won), PNP_CORR_DTYPE), np.zeros(len(won), PROJ_PAIR_DTYPE)
    corr["X"] = g["landmarks"]["X"][f["first"] + won]
    corr["u"], corr["v"] = f["kp"]["x"][k], f["kp"]["y"][k]
    pairs["landmark"], pairs["keypoint"] = f["first"] + won, k
    return obs, corr, pairs


_RESTATED = {}


def edge_restatement(g, f):
    """(obs: land_cap records, corr, pairs) by proj_ref, computed once per frame. A range of more than COMPACT_ABOVE landmarks
    (claim_bits alone) is searched as its live landmarks, compacted in order, and mapped back: a dead landmark is never
    visible, and of i only the order enters a claim."""
    key = (g["name"], f["name"])
    if key not in _RESTATED:
        kp, desc = edge_frame_arrays(g, f)
        lm = g["landmarks"][f["first"]:f["first"] + f["count"]]
        if f["count"] <= COMPACT_ABOVE:
            got = R.search_frame_ref(f["pose"], kp, desc, f["n"], g["kp_stride"], g["landmarks"], f["first"], f["count"], g["land_cap"],
                                     g["cfg"], g["width"], g["height"])[:3]
        else:
            live = np.flatnonzero(lm["octave"] >= 0)
            o, corr, pairs = R.search_ref(f["pose"], kp[:f["n"]], desc[:f["n"]], lm[live], g["cfg"], g["width"], g["height"])
            obs = R.not_visible_obs(g["land_cap"])
            obs[live] = o
            pairs["landmark"] = f["first"] + live[pairs["landmark"]]
            got = (obs, corr, pairs)
        _RESTATED[key] = got
    return _RESTATED[key]
