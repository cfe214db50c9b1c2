"""Hand-made inputs of the sparse stereo stage, one rule of the definition (include/aria_orb_hip.h, "sparse stereo") per
left keypoint, shared by tests/test_stereo_host.py (known answers of the restatement) and tests/test_gpu_stereo.py (the
device against the restatement, as one batch per configuration).

Every left keypoint has a random 256-bit descriptor of its own and the right keypoints meant for it carry the same one, so
keypoints of one pair do not see each other (random descriptors are ~128 bits apart, far above th_hamming = 75)."""
import numpy as np

from aria_slam_amd._lib import KP_DTYPE

W, H = 96, 64
CFG_BOUNDS = dict(min_disparity=4.0, max_disparity=16.0)     # both x bounds reachable inside a 96 px image
CFG_DEFAULT = dict()


def _kps(rows):
    k = np.zeros(len(rows), KP_DTYPE)
    for i, (x, y, o) in enumerate(rows):
        k[i] = (x, y, 31.0, 0.0, 1.0, o)
    return k


def _shifted(left, shift_of_row):
    """right(y, x) = left(y, x + shift[y]), edge-clamped: a keypoint at xL shows at xL - shift."""
    h, w = left.shape
    cols = np.clip(np.arange(w)[None, :] + np.asarray(shift_of_row)[:, None], 0, w - 1)
    return left[np.arange(h)[:, None], cols]


def _case(name, cfg, img_l, img_r, left, right, expect):
    """left: [(x, y, octave)]; right: [(x, y, octave, index of the left keypoint whose descriptor it copies, or None)];
    expect: per left keypoint None (unmatched) or (right index, true disparity or None)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    dl = rng.integers(0, 256, (len(left), 32), dtype=np.uint8)
    dr = np.stack([dl[r[3]] if r[3] is not None else rng.integers(0, 256, 32, dtype=np.uint8) for r in right]) \
        if right else np.zeros((0, 32), np.uint8)
    return dict(name=name, cfg=cfg, img_l=np.ascontiguousarray(img_l), img_r=np.ascontiguousarray(img_r), kp_l=_kps(left),
                desc_l=dl, kp_r=_kps([r[:3] for r in right]), desc_r=dr, expect=expect)


def rule_cases():
    rng = np.random.default_rng(7)
    tex = rng.integers(0, 256, (H, W), dtype=np.uint8)
    # rows 0..15 shifted by 5, 16..47 by 10, 48..63 by 15; every 11-row window below stays inside one band
    shift = np.where(np.arange(H) < 16, 5, np.where(np.arange(H) < 48, 10, 15))
    right = _shifted(tex, shift)
    cases = []

    # ---- step 1: the candidate rules (min_disparity 4, max_disparity 16) ----
    x = np.float32(50.4)
    above = np.nextafter(np.float32(70.4) - np.float32(4.0), np.float32(1e9), dtype=np.float32)
    r1 = right.copy()
    r1[30, 20] += 1 if r1[30, 20] < 255 else -1          # keypoint 8's best SAD is 1: the median filter (med = 0) drops it
    cases.append(_case(
        "candidates", CFG_BOUNDS, tex, r1,
        left=[(60, 30, 0), (60, 24, 0), (60, 36, 0), (70, 30, 0), (70, 36, 0), (x, 56, 0), (x, 8, 0), (70.4, 8, 0), (30, 30, 0)],
        right=[(50, 30, 0, 0), (48, 30, 0, 0),           # duplicate descriptors: the lowest j wins
               (50, 26.0, 0, 1),                         # |dy| = 2.0 = band_factor * scale[0]: accepted
               (50, 38.5, 0, 2),                         # |dy| = 2.5: outside the band
               (60, 30, 2, 3),                           # octave difference 2: excluded
               (60, 36, 1, 4),                           # octave difference 1: accepted
               (x - np.float32(16.0), 56, 0, 5),         # xR == xL - max_disparity: accepted (rows shifted by 15)
               (x - np.float32(4.0), 8, 0, 6),           # xR == xL - min_disparity: accepted (rows shifted by 5)
               (above, 8, 0, 7),                         # one ulp beyond xL - min_disparity: excluded
               (20, 30, 0, 8)],
        expect=[(0, 10.0), (2, 10.0), None, None, (5, 10.0), (6, 15.0), (7, 5.0), None, None]))

    # ---- step 2: windows off the image, best shift at the ends of the slide, flat texture ----
    flat_l, flat_r = tex.copy(), right.copy()
    flat_l[16:48, 0:48] = 90
    flat_r[16:48, 0:48] = 90
    cases.append(_case(
        "slide", CFG_BOUNDS, flat_l, flat_r,
        left=[(92, 30, 0), (70, 3, 0), (19, 56, 0), (80, 30, 0), (80, 42, 0), (30, 30, 0), (75, 36, 0)],
        right=[(82, 30, 0, 0),                           # left window leaves the image on the right
               (60, 3, 0, 1),                            # both windows leave the image at the top
               (9, 56, 0, 2),                            # the slide of the right window leaves the image on the left
               (75, 30, 0, 3),                           # true shift 10 = best inc -5 = -L: unmatched
               (65, 42, 0, 4),                           # best inc +5 = +L: unmatched
               (20, 30, 0, 5),                           # flat texture: every SAD is 0, the lowest inc (-L) wins: unmatched
               (65, 36, 0, 6)],                          # a regular match beside them
        expect=[None, None, None, None, None, None, (6, 10.0)]))

    # ---- step 3: disparity 0 is clamped to 0.01 (default configuration: min_disparity 0) ----
    sym = rng.integers(0, 256, (H, 49), dtype=np.uint8)[:, np.abs(np.arange(W) - 48)]   # symmetric about column 48
    cases.append(_case("clamp", CFG_DEFAULT, sym, sym, left=[(48, 30, 0)], right=[(48, 30, 0, 0)], expect=[(0, 0.0)]))

    # ---- an empty side ----
    cases.append(_case("empty_right", CFG_DEFAULT, tex, right, left=[(60, 30, 0), (70, 36, 0)], right=[], expect=[None, None]))
    cases.append(_case("empty_left", CFG_DEFAULT, tex, right, left=[], right=[(50, 30, 0, None)], expect=[]))
    return cases


def stack_cases(cases, kp_stride):
    """The cases as one batch: (img_l, img_r (n, H, W), kp_l, kp_r (n, kp_stride), desc_l, desc_r (n, kp_stride, 32), n_l, n_r)."""
    n = len(cases)
    il, ir = np.stack([c["img_l"] for c in cases]), np.stack([c["img_r"] for c in cases])
    kl, kr = np.zeros((n, kp_stride), KP_DTYPE), np.zeros((n, kp_stride), KP_DTYPE)
    dl, dr = np.zeros((n, kp_stride, 32), np.uint8), np.zeros((n, kp_stride, 32), np.uint8)
    nl, nr = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for p, c in enumerate(cases):
        nl[p], nr[p] = len(c["kp_l"]), len(c["kp_r"])
        kl[p, :nl[p]], kr[p, :nr[p]] = c["kp_l"], c["kp_r"]
        dl[p, :nl[p]], dr[p, :nr[p]] = c["desc_l"], c["desc_r"]
    return il, ir, kl, kr, dl, dr, nl, nr
