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


# ---- edge groups: every window, pass, chunk, span, bin, count and key the C-ABI admits ------------------------------------------------
# (tests/test_stereo_edges_host.py: the restatement against the written answers and a census of what each group reaches;
#  tests/test_gpu_stereo_edges.py: the device against the restatement, bitwise.)
#
# One group = one configuration, one image size, one kp_stride, one launch. Every pair is built from seeds and carries the
# answer written down from its construction: per left keypoint None (unmatched) or (right index, s) where the disparity lies
# within half a pixel of the integer s (s <= 0: the disparity is the clamp 0.01 exactly; s = None: nothing is claimed).
#
# A textured pair is cut from ONE wider random texture, right(y, x) = left(y, x + d) on every pixel, so a left keypoint at ul
# shows at ul - d and the slide of a right keypoint at ur has its zero SAD at index k = L + (ul - d - ur). A `site` is a left
# keypoint and the right keypoint placed for a chosen k.
#
# Left out on purpose: NaN coordinates. The header does not define them and the restatement raises on them (int(rint(nan))),
# so no case holds one. And `den == 0`: it cannot occur. The best index k is the LOWEST index of the least SAD, so
# SAD(k - 1) > SAD(k) and SAD(k + 1) >= SAD(k), hence den = 2 (d1 + d3 - 2 d2) >= 2. The host test asserts this on every slide.
import functools

from aria_slam_amd import stereo_ref as _R
from aria_slam_amd._lib import MATCH_DTYPE, POSE_RESULT_DTYPE, STEREO_OBS_DTYPE

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
CFG_WIDE = dict(min_disparity=-64.0, max_disparity=64.0)    # both signs of disparity, every x of a 128 px image in range
LDS_DEFAULT = 64 * 1024


def shift_pair(seed, h, w, d, period=None):
    """(left, right) u8, right(y, x) = left(y, x + d) everywhere, d of either sign; period: one period per 16-row band
    (a list, None entries = random), the texture of a band repeating every `period` columns."""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (h, w + abs(d)), dtype=np.uint8)
    for b, p in enumerate(period or []):
        if p:
            base = rng.integers(0, 256, (16, p), dtype=np.uint8)
            big[16 * b:16 * b + 16] = base[:, np.arange(w + abs(d)) % p]
    left, right = (big[:, :w], big[:, d:d + w]) if d >= 0 else (big[:, -d:-d + w], big[:, :w])
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


class _Pair:
    """Builder of one pair. Descriptors: every left keypoint a random one; a right keypoint copies the one of left keypoint
    `of` with its first `flip` bits inverted (Hamming distance = flip exactly), or is random (of=None)."""

    def __init__(self, name, img_l, img_r):
        self.name, self.img_l, self.img_r = name, img_l, img_r
        self.left, self.right, self.expect = [], [], []

    def lkp(self, x, y, o=0, expect=None):
        self.left.append((x, y, o))
        self.expect.append(expect)
        return len(self.left) - 1

    def rkp(self, x, y, o=0, of=None, flip=0):
        self.right.append((x, y, o, of, flip))
        return len(self.right) - 1

    def site(self, ul, v, d, L, k, matched=True, o=(0, 0), flip=0, yr=None, xl=None, xr=None):
        """Left keypoint at (ul, v), right at the ur whose slide has its zero at index k. matched=False: refused by a rule."""
        ur = ul - d + (L - k)
        i = self.lkp(ul if xl is None else xl, v, o[0])
        j = self.rkp(ur if xr is None else xr, v if yr is None else yr, o[1], of=i, flip=flip)
        self.expect[i] = (j, d) if matched and 1 <= k <= 2 * L - 1 else None
        return i, j

    def done(self):
        rng = np.random.default_rng(sum(map(ord, self.name)) + 1000)
        nl, nr = len(self.left), len(self.right)
        dl = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
        dr = rng.integers(0, 256, (nr, 32), dtype=np.uint8)
        for j, (_, _, _, of, flip) in enumerate(self.right):
            if of is not None:
                bits = np.unpackbits(dl[of])
                bits[:flip] ^= 1
                dr[j] = np.packbits(bits)
        kl, kr = np.zeros(nl, KP_DTYPE), np.zeros(nr, KP_DTYPE)
        for k, rows in ((kl, self.left), (kr, self.right)):
            if len(rows):
                k["x"], k["y"] = [r[0] for r in rows], [r[1] for r in rows]
                k["octave"] = [r[2] for r in rows]
                k["size"], k["response"] = 31.0, 1.0
        return dict(name=self.name, img_l=self.img_l, img_r=self.img_r, kp_l=kl, desc_l=dl, kp_r=kr, desc_r=dr,
                    expect=list(self.expect))


def _group(name, cfg, pairs, kp_stride=None, **reach):
    h, w = pairs[0]["img_l"].shape
    assert all(p["img_l"].shape == (h, w) and p["img_r"].shape == (h, w) for p in pairs)
    n = max(max(len(p["kp_l"]), len(p["kp_r"])) for p in pairs)
    kp_stride = kp_stride or max(16, -(-n // 8) * 8 + 8)
    assert n <= kp_stride
    return dict(name=name, kind="match", cfg=cfg, width=w, height=h, kp_stride=kp_stride, pairs=pairs, reach=reach)


# ---- windows ---------------------------------------------------------------------------------------------------------------------
WINDOW_SLIDES = {1: (5, 9), 2: (5, 9), 3: (5, 9), 4: (5, 9), 5: (5, 9), 6: (5, 9), 7: (5, 9, 16)}


def _windows(w, L):
    """128 x 48, shift +-(L + 2). Pair `right` (d > 0): windows touching column W - 1 (left) and column 0 (right slide), rows 0
    and H - 1, each accepted and one pixel further refused, and a dozen sites inside. Pair `left` (d < 0): column 0 (left window)
    and column W - 1 (right slide)."""
    W_, H_, D = 128, 48, L + 2
    cfg = dict(CFG_WIDE, sad_half_window=w, sad_slide=L)
    rng = np.random.default_rng(100 * w + L)
    pairs = []
    for sign in (1, -1):
        d = sign * D
        p = _Pair("windows w=%d L=%d d=%+d" % (w, L, d), *shift_pair(1000 * w + 10 * L + (sign > 0), H_, W_, d))
        n_in = 0
        while n_in < (12 if sign > 0 else 6):
            ur, k, v = int(rng.integers(L + w, W_ - L - w)), int(rng.integers(1, 2 * L)), int(rng.integers(w, H_ - w))
            ul = ur + d - (L - k)
            if w <= ul <= W_ - 1 - w:
                p.site(ul, v, d, L, k)
                n_in += 1
        mid = H_ // 2
        if sign > 0:
            p.site(W_ - 1 - w, mid, d, L, L)                              # the left window ends on column W - 1
            p.site(W_ - w, mid, d, L, L, matched=False)                   # ... one further
            p.site(L + w + d, mid, d, L, L)                               # the right slide starts on column 0
            p.site(L + w + d - 1, mid, d, L, L, matched=False)
            p.site(60, w, d, L, L - 1)                                    # both windows start on row 0
            p.site(60, w - 1, d, L, L - 1, matched=False)
            p.site(70, H_ - 1 - w, d, L, L + 1)                           # ... end on row H - 1
            p.site(70, H_ - w, d, L, L + 1, matched=False)
        else:
            p.site(w, mid, d, L, L)                                       # the left window starts on column 0
            p.site(w - 1, mid, d, L, L, matched=False)
            p.site(W_ - 1 - L - w + d, mid, d, L, L)                      # the right slide ends on column W - 1
            p.site(W_ - L - w + d, mid, d, L, L, matched=False)
        pairs.append(p.done())
    return _group("windows w=%d L=%d" % (w, L), cfg, pairs, window=w, passes=(2 * L + 16) // 16)


# ---- slide -----------------------------------------------------------------------------------------------------------------------
SLIDE_WINDOW = {1: 5, 7: 2, 8: 4, 15: 6, 16: 1}
# (period, lowest zero index): the SAD is zero at lowest + m * period
SLIDE_TIES = {1: [(2, 0)],
              7: [(7, 3), (14, 0), (5, 4)],
              8: [(8, 7), (15, 1), (16, 0), (2, 1)],
              15: [(16, 14), (15, 1), (16, 0), (15, 0)],
              16: [(4, 3), (16, 15), (16, 1), (16, 14), (10, 6), (16, 0), (32, 0)]}


def _slide(L):
    """128 px wide, shift 20. Pair `indices`: one site per index 0..2L, so every best index occurs and the two ends are
    unmatched. Pair `ties`: one 16-row band of periodic texture per entry of SLIDE_TIES[L]; the zero SAD repeats every period and
    the lowest index must win (index 0: unmatched)."""
    w, W_, D = SLIDE_WINDOW[L], 128, 20
    ties = SLIDE_TIES[L]
    H_ = max(64, 16 * len(ties))
    cfg = dict(CFG_WIDE, sad_half_window=w, sad_slide=L)
    p = _Pair("slide L=%d indices" % L, *shift_pair(7000 + L, H_, W_, D))
    for k in range(2 * L + 1):
        ur = L + w + (3 * k) % 20
        p.site(ur + D - (L - k), w + k % (H_ - 2 * w), D, L, k)
    q = _Pair("slide L=%d ties" % L, *shift_pair(7100 + L, H_, W_, D, period=[t[0] for t in ties]))
    for b, (per, k0) in enumerate(ties):
        assert 0 <= k0 < per and k0 + per <= 2 * L
        ur = L + w + 2
        q.site(ur + D - (L - k0), 16 * b + 8, D, L, k0)
    return _group("slide L=%d" % L, cfg, [p.done(), q.done()], indices=set(range(2 * L + 1)), ties=ties)


# ---- rows ------------------------------------------------------------------------------------------------------------------------
ROW_HEIGHTS = (3, 255, 256, 257, 480, 4096)
CFG_ROWS = dict(sad_half_window=2, sad_slide=5)                   # also the configuration of `counts`: one handle, three shapes


def chunk_rows(h):
    """First and last row of every thread's chunk of the kernel's row scan (chunk = ceil(H / 256) rows per thread)."""
    c = -(-h // 256)
    return sorted({r for t in range(256) if t * c < h for r in (t * c, min(t * c + c, h) - 1)})


def _rows(h):
    """96 x h, shift 8, band 2 (octave 0). A site on every row of chunk_rows(h): matched where the window fits. And probes: a
    left keypoint on row Y whose one true candidate sits on the band's edge (Y + 2 or Y - 2) at distance 3, with exact copies
    of its descriptor on the rows lo = Y - 4, lo - 1, hi = Y + 3 and hi + 1 of the kernel's span (the widest band of the allowed
    octaves is 2 * 1.2 rows, and one row of slack) and on Y - 3: outside the band of octave 0, they lose."""
    w = 1 if h == 3 else 2
    L, D, W_ = 5, 8, 96
    cfg = dict(CFG_ROWS, sad_half_window=w)
    p = _Pair("rows H=%d" % h, *shift_pair(9000 + h, h, W_, D))
    for r in chunk_rows(h):
        k = 1 + r % (2 * L - 1)
        ur = 10 + (7 * r) % 60
        p.site(ur + D - (L - k), r, D, L, k, matched=w <= r <= h - 1 - w)
    probes = []
    if h > 16:
        c = -(-h // 256)
        probes = sorted({2, 5, h // 2, h - 6, h - 3} | {y for y in (255, 256, 257, 100 * c - 1, 100 * c, 100 * c + c - 1) if 5 < y < h - 6})
    for n, y in enumerate(probes):
        ul = 30 + 5 * (n % 10)
        i = p.lkp(ul, y)
        true_row = y + 2 if (y + 2 <= h - 1 and n % 2 == 0) or y - 2 < 0 else y - 2
        for row in (y - 5, y - 4, y - 3, y + 3, y + 4):
            if 0 <= row < h:
                p.rkp(ul - D, row, of=i)
        p.expect[i] = (p.rkp(ul - D, true_row, of=i, flip=3), D)
    return _group("rows H=%d" % h, cfg, [p.done()], kp_stride=640 if h > 16 else 16, chunk=-(-h // 256), probes=probes)


# ---- span ------------------------------------------------------------------------------------------------------------------------
SPAN_ROWS = (2000, 2005)                                          # 8192 right keypoints on rows 2000..2005 of 4096
SPAN_FIRST, SPAN_LAST = 4000, (17, 5000, 8191)                    # the only keypoint of row 2000; the three of row 2005
CFG_SPAN = dict(min_disparity=-200.0, max_disparity=200.0, sad_half_window=2, sad_slide=5)


def span_row(j):
    return 2000 if j == SPAN_FIRST else 2005 if j in SPAN_LAST else 2001 + j % 4


def _span():
    """96 x 4096, kp_stride 8192: the 147,456-byte launch. Every right keypoint is a candidate by x of every left keypoint; the
    left keypoints sit on rows 2002..2005, so a span (rows y - 4 .. y + 3) is all 8192 (128 full steps of 64) or, from row
    2005, 8191 (the last step partial). Row 2000 holds j = 4000 alone: sorted slot 0, the first lane of the first step. Row 2005 holds j = 17, 5000 and
    8191: the last three slots. Elsewhere the order inside a row is free, and the winner must not depend on it."""
    W_, H_, L, D = 96, 4096, 5, 8
    rng = np.random.default_rng(4242)
    p = _Pair("span 8192", *shift_pair(4243, H_, W_, D))
    xr = rng.integers(7, 89, 8192).astype(np.float64)
    owner = [None] * 8192                                         # (left index, flip)

    def claim(j, yl, flip=0, winner=True):
        k = 1 + int(rng.integers(0, 2 * L - 1))
        ur = int(rng.integers(L + 2, W_ - L - 2 - D))
        i = p.lkp(ur + D - (L - k), yl)
        xr[j], owner[j] = ur, (i, flip)
        p.expect[i] = (j, D)
        return i

    claim(SPAN_FIRST, 2002)                                       # the winner in the first lane of the first step
    claim(8191, 2005)                                             # ... in the last, partial step, and the greatest j
    claim(17, 2005)
    claim(5000, 2003)
    ties = ((6003, 6100, 8001), (103, 4102, 7001), (7777, 7776), (2, 8190))
    taken = {SPAN_FIRST, *SPAN_LAST} | {j for js in ties for j in js}
    for j in rng.permutation(8192):
        if len(p.left) >= 560:
            break
        if int(j) not in taken:
            taken.add(int(j))
            claim(int(j), float(np.clip(span_row(int(j)) + int(rng.integers(-1, 2)), 2002, 2003)))
    # equal distances on different j, rows and steps: the lowest j wins wherever it was sorted to
    for js in ties:
        i = claim(min(js), 2003, flip=4)
        for j in js:
            if j != min(js):
                xr[j], owner[j] = xr[min(js)], (i, 4)
    for j in range(8192):
        of, flip = owner[j] if owner[j] else (None, 0)
        p.rkp(float(xr[j]), span_row(j), of=of, flip=flip)
    one = _Pair("span twin", *shift_pair(4243, H_, W_, D))
    one.site(40, 2002, D, L, 4)
    return [_group("span 8192", CFG_SPAN, [p.done()], kp_stride=8192, lds=147456),
            _group("span twin kp_stride=1", CFG_SPAN, [one.done()], kp_stride=1, lds=(4096 + 4) * 4)]


# ---- median ----------------------------------------------------------------------------------------------------------------------
def _median_pair(name, sads, keep, flat=False):
    """w = 7, L = 5, 96 px wide, one 15-row band per keypoint. The left image is 0, the right image 255 but for one 15 x 15 block
    per band whose pixels sum to the prescribed SAD, its deficit to 255 taken from the LAST column backwards: a window further
    left loses that column for one of 255 (a strictly greater SAD), a window further right can at best tie, and ties go to the
    lower index. So the surviving SAD of keypoint i is sads[i] exactly (at most 57374 = 15 * 15 * 255 - 1). flat: one more
    keypoint without a block, all 33... all 11 SADs 57375, the best index 0: unmatched."""
    n = len(sads) + (1 if flat else 0)
    left, right = np.zeros((90, 96), np.uint8), np.full((90, 96), 255, np.uint8)
    assert n <= 6
    p = _Pair(name, left, right)
    for i in range(n):
        k = 3 + i % 5
        ur, ul, v = 40, 48, 15 * i + 7
        ub = ur + (k - 5)
        if i < len(sads):
            assert 0 <= sads[i] <= 57374
            deficit = 57375 - sads[i]
            block = np.full(225, 255, np.int64)
            for c in range(225):                                  # column-major from the last column
                take = min(255, deficit)
                block[c] -= take
                deficit -= take
            right[v - 7:v + 8, ub - 7:ub + 8] = block.reshape(15, 15).T[:, ::-1]
        a = p.lkp(ul, v)
        j = p.rkp(ur, v, of=a)
        p.expect[a] = (j, ul - ub) if i < len(sads) and keep[i] else None
    return p.done()


def _median():
    cfg = dict(sad_half_window=7, sad_slide=5)
    main = [_median_pair("median n=1, bin 0, rank 0", [3], [1]),
            _median_pair("median n=2", [9, 3], [1, 1]),
            _median_pair("median n=3", [100, 3, 9], [0, 1, 1]),
            _median_pair("median bin 156, first of its bin", [40001, 10, 40002, 20, 40000], [1, 1, 1, 1, 1]),
            _median_pair("median last of its bin", [600, 259, 257, 700, 258], [0, 1, 1, 0, 1]),
            _median_pair("median all equal", [77, 77, 77, 77], [1, 1, 1, 1]),
            _median_pair("median the largest SAD alone", [57374], [1], flat=True),
            _median_pair("median the largest SAD as the median", [57374, 100, 57374], [1, 1, 1], flat=True),
            _median_pair("median (float)sad == 2.1f * 10 = 21 in fp32", [21, 10, 22, 10, 10], [1, 1, 0, 1, 1])]
    return [_group("median", cfg, main, bins={0, 1, 156, 224}),
            _group("median factor 2.5", dict(cfg, median_factor=2.5), [_median_pair("median 10 == 2.5 * 4", [4, 10, 4, 11, 4], [1, 1, 1, 0, 1])]),
            _group("median factor 0", dict(cfg, median_factor=0.0), [_median_pair("median factor 0 keeps zeros", [0, 5, 0, 7, 0], [1, 0, 1, 0, 1]),
                                                                      _median_pair("median factor 0 drops all", [1, 2, 3], [0, 0, 0])])]


# ---- rule ends -------------------------------------------------------------------------------------------------------------------
def _ends_pair(name, sites, L=5, D=8, seed=0):
    """96 x 32, w = 2, shift 8. sites: dicts for _Pair.site beyond (ul, v, d, L, k); ul, v and k default to a free place."""
    p = _Pair(name, *shift_pair(5000 + seed, 32, 96, D))
    for n, s in enumerate(sites):
        s = dict(s)
        ul, v, k = s.pop("ul", 20 + 6 * (n % 11)), s.pop("v", 4 + 6 * (n % 5)), s.pop("k", 1 + n % 9)
        p.site(ul, v, D, L, k, **s)
    return p.done()


def _ends():
    w2 = dict(sad_half_window=2, sad_slide=5)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(1e9)))   # noqa: E731
    octs = lambda rows: [dict(o=(a, b), matched=m) for a, b, m in rows]   # noqa: E731
    groups = []
    default = octs([(-3, -3, 1), (-3, -4, 1), (-3, -5, 0), (9, 9, 1), (9, 10, 1), (9, 11, 0), (INT_MAX, INT_MAX, 1),
                    (INT_MIN, INT_MIN, 1), (INT_MAX, INT_MIN, 0), (INT_MIN, INT_MAX, 0), (INT_MAX, INT_MAX - 1, 1), (INT_MIN + 1, INT_MIN, 1)])
    default += [dict(flip=74), dict(flip=75, matched=False),                               # th_hamming - 1 and th_hamming
                # round-half-even: xR 6.5 -> 6 (the slide leaves column 0), 7.5 -> 8; xL 93.5 -> 94 (leaves column 95), 92.5 -> 92
                dict(ul=6 + 8, k=5, xr=6.5, matched=False), dict(ul=8 + 8, k=5, xr=7.5),
                dict(ul=94, k=5, xl=93.5, matched=False), dict(ul=92, k=5, xl=92.5),
                # |x| above 1e6, and beyond int32: a candidate by every rule of step 1, refused by the window
                dict(xl=2.0e6, xr=2.0e6 - 8, matched=False), dict(xl=-2.0e6, xr=-2.0e6 - 8, matched=False), dict(xl=3.0e9, xr=3.0e9, matched=False),
                dict(v=2, yr=0.0), dict(v=29, yr=31.0)]                                    # a candidate on row 0 and on row H - 1
    groups.append(_group("ends default", w2, [_ends_pair("ends default", default)]))
    # yL 0.5 -> 0 and 29.5 -> 30 leave the image, 1.5 -> 2, 2.5 -> 2 and 28.5 -> 28 do not (w = 2, H = 32)
    ys = [dict(v=y, yr=y, matched=m) for y, m in ((0.5, 0), (1.5, 1), (2.5, 1), (28.5, 1), (29.5, 0))]
    groups.append(_group("ends rounding of y", w2, [_ends_pair("ends rounding of y", ys, seed=1)]))
    band4 = [dict(v=2.0, yr=-1.5), dict(v=29.0, yr=32.5), dict(v=29.0, yr=33.5, matched=False), dict(v=2.0, yr=-1000.0, matched=False),
             dict(v=-0.4, yr=-0.4, matched=False), dict(v=10.0, yr=14.0), dict(v=16.0, yr=up(20.0), matched=False),
             dict(v=22.0, yr=22.0 + 4.0 * 1.2, o=(0, 1)), dict(v=5.0, yr=5.0 + 4.0 * 1.44 + 0.01, o=(1, 2), matched=False)]
    groups.append(_group("ends band_factor=4", dict(w2, band_factor=4.0), [_ends_pair("ends band 4", band4, seed=2)]))
    groups.append(_group("ends band_factor=0", dict(w2, band_factor=0.0),
                         [_ends_pair("ends band 0", [dict(v=4.25, yr=4.25), dict(v=10.25, yr=up(10.25), matched=False), dict(v=16.0, yr=16.0, o=(7, 8))], seed=3)]))
    groups.append(_group("ends band_factor=1e9", dict(w2, band_factor=1.0e9),
                         [_ends_pair("ends band 1e9", [dict(v=5, yr=31.0), dict(v=20, yr=1.0e8), dict(v=26, yr=-3.0e7), dict(v=3, yr=0.0)], seed=4)]))
    groups.append(_group("ends max_octave_diff=0", dict(w2, max_octave_diff=0),
                         [_ends_pair("ends mod 0", octs([(0, 0, 1), (0, 1, 0), (3, 3, 1), (INT_MAX, INT_MAX, 1), (-1, 0, 0), (INT_MIN, INT_MAX, 0)]), seed=5)]))
    groups.append(_group("ends max_octave_diff=8", dict(w2, max_octave_diff=8),
                         [_ends_pair("ends mod 8", octs([(0, 8, 1), (0, 9, 0), (7, -1, 1), (7, -2, 0), (INT_MAX, INT_MIN, 0), (INT_MIN, INT_MIN + 8, 1),
                                                        (INT_MIN, INT_MIN + 9, 0), (INT_MAX - 8, INT_MAX, 1)]), seed=6)]))
    groups.append(_group("ends th_hamming=0", dict(w2, th_hamming=0), [_ends_pair("ends th 0", [dict(matched=False)], seed=7)]))
    groups.append(_group("ends th_hamming=257", dict(w2, th_hamming=257), [_ends_pair("ends th 257", [dict(flip=256)], seed=8)]))
    groups.append(_group("ends th_hamming=256", dict(w2, th_hamming=256),
                         [_ends_pair("ends th 256: 256", [dict(flip=256, matched=False)], seed=9), _ends_pair("ends th 256: 255", [dict(flip=255)], seed=10)]))
    return groups


# ---- counts ----------------------------------------------------------------------------------------------------------------------
COUNTS_DENSE, COUNTS_ABSENT = (0, 5, 31), (1, 2, 30)              # rounds of 256 left keypoints of the nL = 8192 pair


def _counts_pair(name, nl, nr, alive):
    """96 x 64, shift 8: nr right keypoints, each the match of every left keypoint i with alive(i) that is placed on it
    (i % nr); the other left keypoints carry a descriptor nobody copies (unmatched by th_hamming)."""
    L, D = 5, 8
    p = _Pair(name, *shift_pair(6000, 64, 96, D))
    spots = [(20 + 4 * s, 4 + 3 * s, 1 + s % 9) for s in range(nr)]
    first = {}
    for i in range(nl):
        ul, v, k = spots[i % nr]
        p.lkp(ul, v)
        if alive(i):
            first.setdefault(i % nr, i)
    for s, (ul, v, k) in enumerate(spots):
        p.rkp(ul - D + (L - k), v, of=first.get(s))
    out = p.done()
    for i in range(nl):
        if alive(i):
            out["desc_l"][i] = out["desc_l"][first[i % nr]]
            out["expect"][i] = (i % nr, D)
    return out


def _counts():
    small = [_counts_pair("counts nL=%d" % n, n, 8, lambda i: i % 3 != 0) for n in (15, 16, 17, 255, 256, 257)]
    big = _counts_pair("counts nL=8192", 8192, 16,
                       lambda i: i // 256 in COUNTS_DENSE or (i // 256 not in COUNTS_ABSENT and i % 5 == 0))
    return [_group("counts", CFG_ROWS, small, kp_stride=264), _group("counts nL=8192", CFG_ROWS, [big], kp_stride=8192, lds=(64 + 4 * 8192) * 4)]


@functools.lru_cache(maxsize=None)
def edge_groups():
    """The match groups, built once per process. Nobody writes into them."""
    g = [_windows(w, L) for w, Ls in WINDOW_SLIDES.items() for L in Ls]
    g += [_slide(L) for L in SLIDE_TIES]
    g += [_rows(h) for h in ROW_HEIGHTS]
    g += _span() + _median() + _ends() + _counts()
    assert len({x["name"] for x in g}) == len(g)
    return tuple(g)


def edge_group(name):
    return next(g for g in edge_groups() + scale_groups() if g["name"] == name)


@functools.lru_cache(maxsize=None)
def edge_restatement(name, p):
    """(obs, matches) of pair p of the group, computed once per process."""
    g = edge_group(name)
    c = g["pairs"][p]
    return _R.stereo_match_ref(c["img_l"], c["img_r"], c["kp_l"], c["desc_l"], c["kp_r"], c["desc_r"], **g["cfg"])


def match_lds_bytes(g):
    """Dynamic LDS of the group's launch: 4 bytes per image row and 16 per keypoint of kp_stride."""
    return 4 * g["height"] + 16 * g["kp_stride"]


# ---- scale -----------------------------------------------------------------------------------------------------------------------
def order_key(x):
    """The kernel's 64-bit key of an fp64: unsigned order = numeric order."""
    b = int(np.float64(x).view(np.uint64))
    return (~b & (2 ** 64 - 1)) if b >> 63 else b | 1 << 63


def first_differing_byte(values):
    """The most significant byte (0 = highest) in which the keys of the values are not all equal."""
    keys = [order_key(v) for v in values]
    return next(k for k in range(8) if len({key >> (56 - 8 * k) & 255 for key in keys}) > 1)


def _scale_record(name, s, min_matches=5, mask=None, dead=(), pose_valid=1, form="plain", A=None, byte=None, rot=False):
    """One record whose s_m are the prescribed fp64 values `s`, exactly. View 1 holds X1, view 2 X2, match m joins keypoint m of
    both (in a shuffled order of the keypoints).
      plain: t = (0, 0, 1), X1 = 0 (rot: a quarter turn about z and small integer X1), X2.z = s (fp32-exact values);
      zeros: t = (1, 1, 1), X2 = (+-0, +-0, s) with the sign of s, so that -0.0 arrives as -0.0;
      ulps:  t = (A, 2^(8 (7 - byte)) ulp, 0), X2 = (1, c, 0): s = A + c 2^(8 (7 - byte)) ulp(A) for integer c, exact in fp64.
    dead: matches whose view-1 observation is unmatched; mask: bytes or None (every match)."""
    n = len(s)
    rng = np.random.default_rng(sum(map(ord, name)))
    o1, o2 = _R.unmatched_obs(n), _R.unmatched_obs(n)
    o1["right_idx"] = o2["right_idx"] = 0
    for f in ("X", "Y", "depth"):
        o1[f] = o2[f] = 0.0
    R, t = np.eye(3), np.array([0.0, 0.0, 1.0])
    sv = np.asarray(s, np.float64)
    if form == "plain":
        assert (sv.astype(np.float32).astype(np.float64) == sv).all()
        o2["depth"] = sv
        if rot:
            R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
            X1 = rng.integers(-8, 9, (n, 3)).astype(np.float64)
            o1["X"], o1["Y"], o1["depth"] = X1[:, 0], X1[:, 1], X1[:, 2]
            o2["X"], o2["Y"], o2["depth"] = -X1[:, 1], X1[:, 0], X1[:, 2] + sv
            assert (o2["depth"].astype(np.float64) == X1[:, 2] + sv).all()
    elif form == "zeros":
        t = np.array([1.0, 1.0, 1.0])
        o2["X"] = o2["Y"] = np.copysign(0.0, sv)
        o2["depth"] = sv
    else:
        unit = 2.0 ** (8 * (7 - byte) - 52)
        c = (sv - A) / unit
        assert (c == np.rint(c)).all() and (np.abs(c) < 2 ** 24).all() and (A + c * unit == sv).all()
        t = np.array([A, unit, 0.0])
        o2["X"], o2["Y"] = 1.0, c
    for m in dead:
        o1[m] = _R.unmatched_obs(1)[0]
    perm1, perm2 = rng.permutation(n), rng.permutation(n)
    q1, q2 = _R.unmatched_obs(n), _R.unmatched_obs(n)
    q1[perm1], q2[perm2] = o1, o2
    pose = np.zeros((), POSE_RESULT_DTYPE)
    pose["R"], pose["t"], pose["valid"] = R.ravel(), t, pose_valid
    mk = np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8)
    used = sorted(float(sv[m]) for m in range(n) if mk[m] and m not in set(dead)) if pose_valid else []
    want = (1.0, len(used), 0)
    if len(used) >= max(min_matches, 1) and used[len(used) // 2] > 0:
        want = (used[len(used) // 2], len(used), 1)
    return dict(name=name, pose=pose, idx1=perm1, idx2=perm2, obs1=q1, obs2=q2, mask=mk, s=sv, used=used, expect=want)


SCALE_A = 1.0 + 0x3A5C96E1B7D29 * 2.0 ** -52                      # the mantissa bytes of A: (x3) A5 C9 6E 1B 7D 29


def _scale_records():
    rng = np.random.default_rng(77)
    recs = [_scale_record("key byte 0", [2.0 ** e * sg for e in (-120, -60, 60, 120) for sg in (1, -1)] + [1.0]),
            _scale_record("key byte 1", [1.0 + m / 16.0 for m in range(16)] + [0.5, 0.25])]
    for k in range(2, 8):
        bits = np.float64(SCALE_A).view(np.uint64) & ~np.uint64(255 << (8 * (7 - k)))       # byte k of A cleared: no carry
        A = float(np.uint64(bits).view(np.float64))
        c = rng.permutation(256)[:11]
        recs.append(_scale_record("key byte %d" % k, [A + int(x) * 2.0 ** (8 * (7 - k) - 52) for x in c], form="ulps", A=A, byte=k))
    recs += [_scale_record("median negative", [4.0, -1.0, -5.0, 2.0, -3.0]),
             _scale_record("median zero", [4.0, 0.0, -5.0, 2.0, -3.0]),
             _scale_record("median positive", [4.0, 1.0, -5.0, 2.0, -3.0], rot=True),
             _scale_record("signed zeros", [0.0, -1.0, -0.0, 2.0, 0.0], form="zeros"),
             _scale_record("signed zeros below a positive median", [-0.0, 3.0, 0.0, 2.0, 7.0], form="zeros"),
             _scale_record("ties around the rank", [2.0, 1.0, 2.0, 3.0, 2.0, 2.0, 0.5]),
             _scale_record("ties: the rank is the first of the upper run", [1.0, 2.0, 1.0, 2.0, 1.0, 2.0]),
             _scale_record("all equal", [5.0] * 6),
             _scale_record("even n", [4.0, 1.0, 3.0, 2.0, 6.0, 5.0]),
             _scale_record("odd n", [4.0, 1.0, 3.0, 2.0, 6.0, 5.0, 7.0], rot=True),
             _scale_record("n_used = min_scale_matches - 1", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], mask=[1, 1, 0, 1, 1, 1], dead=[4]),
             _scale_record("n_used = min_scale_matches", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], mask=[1, 1, 0, 1, 1, 1, 1], dead=[4]),
             _scale_record("invalid pose record", [1.0, 2.0, 3.0, 4.0, 5.0], pose_valid=0),
             _scale_record("no match", [])]
    n = 1000
    s = (rng.permutation(n) + 1.0) * 0.25
    mask = np.array([0 if (256 <= m < 512 or m >= 768 or m % 7 == 0) else 1 for m in range(n)], np.uint8)
    recs.append(_scale_record("mask removes whole rounds", s, mask=mask, dead=[m for m in range(n) if m % 11 == 0], rot=True))
    return recs


def _scale_group(name, recs, cap, qf, with_mask=True):
    return dict(name=name, kind="scale", cfg=dict(min_scale_matches=5), match_cap=cap, kp_stride=cap, query_is_first=qf,
                with_mask=with_mask, records=recs)


@functools.lru_cache(maxsize=None)
def scale_groups():
    rng = np.random.default_rng(78)
    full = [_scale_record("n = match_cap = 8192", (rng.permutation(8192) - 3000.0) * 0.25, rot=True),
            _scale_record("n = 8191, median negative", (rng.permutation(8191) - 5000.0) * 0.25)]
    return (_scale_group("scale, query is view 1", _scale_records(), 1100, True),
            _scale_group("scale, query is view 2", _scale_records(), 1100, False),
            _scale_group("scale match_cap=8192", full, 8192, True, with_mask=False))


def scale_arrays(g):
    """The group as the batch arrays of aria_stereo_scale_batch_device: (pose (n,), mask (n, cap), matches (n, cap), nm (n,),
    obs_query (n, cap), nq (n,), obs_train (n, cap), nt (n,))."""
    recs, cap = g["records"], g["match_cap"]
    n = len(recs)
    pose = np.zeros(n, POSE_RESULT_DTYPE)
    mask, m, nm = np.zeros((n, cap), np.uint8), np.zeros((n, cap), MATCH_DTYPE), np.zeros(n, np.int32)
    oq, ot = np.zeros((n, cap), STEREO_OBS_DTYPE), np.zeros((n, cap), STEREO_OBS_DTYPE)
    for p, r in enumerate(recs):
        k = len(r["s"])
        pose[p], nm[p] = r["pose"], k
        mask[p, :k] = r["mask"]
        a, b = (r["idx1"], r["idx2"]) if g["query_is_first"] else (r["idx2"], r["idx1"])
        m[p, :k]["query_idx"], m[p, :k]["train_idx"] = a, b
        oq[p, :k], ot[p, :k] = (r["obs1"], r["obs2"]) if g["query_is_first"] else (r["obs2"], r["obs1"])
    return pose, mask, m, nm.copy(), oq, nm.copy(), ot, nm.copy()


def scale_restatement(g, p):
    pose, mask, m, nm, oq, nq, ot, nt = scale_arrays(g)
    return _R.stereo_scale_ref(pose[p], mask[p, :nm[p]] if g["with_mask"] else None, m[p, :nm[p]], oq[p, :nq[p]], ot[p, :nt[p]],
                               query_is_first=g["query_is_first"], min_scale_matches=g["cfg"]["min_scale_matches"])
