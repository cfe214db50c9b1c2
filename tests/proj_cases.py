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
