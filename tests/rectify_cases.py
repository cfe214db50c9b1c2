"""Shared inputs of the rectification tests (test_rectify_host.py, test_rectify_kernel_emulation.py, test_gpu_rectify.py,
test_cpp_rectify.py): the EuRoC MH cam0 / cam1 calibration as their sensor.yaml files state it, the shapes (a)-(d) the
device tests and the kernel emulation both run, the cases that reach every read form, frame group and limit of the remap
kernel (EDGE_CASES, with read_forms to prove it) and the points cases with non-finite keypoints and cameras that look away,
and the restatement's results on all of them, computed once per process."""
import functools
import math

import numpy as np

from aria_slam_amd import rectify_ref as R
from aria_slam_amd._lib import KP_DTYPE

# EuRoC MH_01 mav0/cam0/sensor.yaml and mav0/cam1/sensor.yaml
T_BS_L = [0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975,
          0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768,
          -0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949,
          0.0, 0.0, 0.0, 1.0]
T_BS_R = [0.0125552670891, -0.999755099723, 0.0182237714554, -0.0198435579556,
          0.999598781151, 0.0130119051815, 0.0251588363115, 0.0453689425024,
          -0.0253898008918, 0.0179005838253, 0.999517347078, 0.00786212447038,
          0.0, 0.0, 0.0, 1.0]
K_L = (458.654, 457.296, 367.215, 248.375)
K_R = (457.587, 456.134, 379.999, 255.238)
D_L = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
D_R = (-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05)
SIZE = (752, 480)
EUROC = dict(K_l=K_L, K_r=K_R, D_l=D_L, D_r=D_R, T_BS_l=T_BS_L, T_BS_r=T_BS_R, size=SIZE)

# shape (a2) / (b): 752x480 -> 637x399, zoomed out so the border is invalid and every fraction occurs
SMALL = (637, 399)
SMALL_NEW_K = (0.6 * (K_L[1] + K_R[1]) / 2, 0.6 * (K_L[1] + K_R[1]) / 2, 321.25, 196.5)
N_FRAMES = 5
SRC_PITCH, SRC_STRIDE = 768, 768 * 480 + 96
DST_PITCH, DST_STRIDE = 641, 641 * 399 + 37
FILL = 7
KP_STRIDE = 300


@functools.lru_cache(maxsize=None)
def cameras(new_K=None):
    """(left camera, right camera, new_K, baseline) of the EuRoC rig by the restatement."""
    return R.rectified_cameras(EUROC, new_K)


@functools.lru_cache(maxsize=None)
def ref_maps(small):
    """The restatement's maps of both cameras: 752x480 -> 752x480 with the default new K, or -> 637x399 with SMALL_NEW_K."""
    cl, cr, nk, _ = cameras(SMALL_NEW_K if small else None)
    dst = SMALL if small else SIZE
    maps = tuple(R.build_map(c, nk, SIZE[0], SIZE[1], dst[0], dst[1]) for c in (cl, cr))
    for m in maps:
        m.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def noise_frames():
    """Shape (b)'s sources: N_FRAMES uniform-noise images per camera, (2, N_FRAMES, 480, 752)."""
    f = np.random.default_rng(20).integers(0, 256, (2, N_FRAMES, SIZE[1], SIZE[0]), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def ref_remapped():
    """The restatement on shape (b): (2, N_FRAMES, 399, 637)."""
    out = np.stack([R.remap(noise_frames()[c], ref_maps(True)[c], FILL) for c in range(2)])
    out.setflags(write=False)
    return out


def padded(imgs, pitch, stride, pad=0xA5):
    """(n, H, W) images in a pitched, strided buffer whose padding is `pad`."""
    n, h, w = imgs.shape
    out = np.full((n, stride), pad, np.uint8)
    out[:, :pitch * h].reshape(n, h, pitch)[:, :, :w] = imgs
    return out


def unpadded(buf, n, h, w, pitch, stride):
    """(images (n, h, w), mask of the padding bytes) of a pitched, strided buffer."""
    buf = np.asarray(buf, np.uint8).reshape(n, stride)
    is_pad = np.ones((n, stride), bool)
    is_pad[:, :pitch * h].reshape(n, h, pitch)[:, :, :w] = False
    # the last row is only w bytes long in a buffer of stride < pitch * h; here stride >= pitch * h always
    return buf[:, :pitch * h].reshape(n, h, pitch)[:, :, :w].copy(), is_pad


@functools.lru_cache(maxsize=None)
def keypoints():
    """Shape (d): three frames of KP_STRIDE records with counts 0, 1 and KP_STRIDE, spread to the image corners; every field
    other than x, y holds its own pattern."""
    rng = np.random.default_rng(21)
    k = np.zeros((3, KP_STRIDE), KP_DTYPE)
    k["x"] = rng.uniform(0, SIZE[0] - 1, (3, KP_STRIDE)).astype(np.float32)
    k["y"] = rng.uniform(0, SIZE[1] - 1, (3, KP_STRIDE)).astype(np.float32)
    corners = [(0, 0), (SIZE[0] - 1, 0), (0, SIZE[1] - 1), (SIZE[0] - 1, SIZE[1] - 1), (SIZE[0] / 2, 0.25), (0.5, SIZE[1] / 2)]
    for f in range(3):
        for j, (x, y) in enumerate(corners):
            k["x"][f, j], k["y"][f, j] = x, y
    k["size"] = rng.uniform(20, 80, (3, KP_STRIDE)).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, (3, KP_STRIDE)).astype(np.float32)
    k["response"] = rng.uniform(0, 1, (3, KP_STRIDE)).astype(np.float32)
    k["octave"] = rng.integers(0, 8, (3, KP_STRIDE))
    k.setflags(write=False)
    return k, np.array([0, 1, KP_STRIDE], np.int32)


def ref_points(cam, kp, counts):
    """The restatement of step 4 on (frames, stride) records: records at and beyond a frame's count stay as they are."""
    cl, cr, nk, _ = cameras(None)
    out = kp.copy()
    for f, n in enumerate(counts):
        if 0 <= n <= kp.shape[1]:
            out[f, :n] = R.undistort_points(kp[f, :n], (cl, cr)[cam], nk)
    return out


def write_sensor_yaml(path, K, D, T_BS, size=SIZE):
    """A sensor.yaml in EuRoC's layout."""
    t = ["%.17g" % v for v in T_BS]
    with open(path, "w") as f:
        f.write("# General sensor definitions.\nsensor_type: camera\ncomment: VI-Sensor cam\n\n"
                "# Sensor extrinsics wrt. the body-frame.\nT_BS:\n  cols: 4\n  rows: 4\n"
                "  data: [%s,\n         %s,\n         %s,\n         %s]\n\n" % tuple(", ".join(t[4 * r:4 * r + 4]) for r in range(4)))
        f.write("# Camera specific definitions.\nrate_hz: 20\nresolution: [%d, %d]\ncamera_model: pinhole\n" % tuple(size))
        f.write("intrinsics: [%s] #fu, fv, cu, cv\n" % ", ".join("%.17g" % v for v in K))
        f.write("distortion_model: radial-tangential\ndistortion_coefficients: [%s]\n" % ", ".join("%.17g" % v for v in D))


# ---- the read forms and edges of k_rect_remap ----------------------------------------------------------------------------
# Cases chosen so that every branch of the kernel's per-lane choice, its frame-group loop and its limits runs, on the device
# (test_gpu_rectify.py, tools/rect_check.py) and through the kernel text compiled for the host
# (test_rectify_kernel_emulation.py). read_forms() proves that a case reaches a branch; test_rectify_host.py asserts it.
NONE, ROWS, TAPS = 0, 1, 2
TILE_W, TILE_H = 64, 16                                        # destination tile of a workgroup
LDS_BYTES = 16384                                              # what k_rect_remap_lds stages at most
EDGE_FRAMES = 17                                               # frame groups of 8, 8 and 1


def rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return (c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0)


def rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return (c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c)


def read_forms(rmap, src_w):
    """The per-lane choice of k_rect_remap as its header comment states it, on a (dst_h, dst_w) map. A lane is four
    horizontally adjacent words of a row padded with invalid words to a multiple of four. Returns a dict of (dst_h, lanes)
    arrays: form (NONE: no valid pixel; ROWS: the valid pixels' upper-left taps span at most 7 columns and 2 rows, so that
    all taps lie within 8 columns and 3 rows, and the 8 columns from the leftmost tap are inside the image; TAPS: otherwise),
    xspan / yspan (largest minus smallest column / row of the valid upper-left taps, -1 for NONE), x0 / y0 (the smallest
    column / row), edge_only (TAPS by the right-edge term alone) and mixed (valid and invalid pixels in one lane). It proves
    that a case reaches a branch; it never computes an expected pixel."""
    m = np.asarray(rmap, np.uint32)
    h, w = m.shape
    lanes = (w + 3) // 4
    p = np.full((h, lanes * 4), R.INVALID, np.uint32)
    p[:, :w] = m
    p = p.reshape(h, lanes, 4)
    ok = p != R.INVALID
    ix, iy = ((p & 0xFFFF) >> 5).astype(np.int64), (p >> 21).astype(np.int64)
    big = 1 << 30
    x0, x1 = np.where(ok, ix, big).min(axis=2), np.where(ok, ix, -1).max(axis=2)
    y0, y1 = np.where(ok, iy, big).min(axis=2), np.where(ok, iy, -1).max(axis=2)
    some = ok.any(axis=2)
    spans_fit = some & (x1 - x0 <= 6) & (y1 - y0 <= 1)
    inside = x0 + 7 <= src_w - 1
    form = np.where(some, np.where(spans_fit & inside, ROWS, TAPS), NONE)
    return dict(form=form, xspan=np.where(some, x1 - x0, -1), yspan=np.where(some, y1 - y0, -1), x0=np.where(some, x0, -1),
                y0=np.where(some, y0, -1), edge_only=spans_fit & ~inside, mixed=some & ~ok.all(axis=2))


def tile_box_bytes(rmap):
    """Bytes of the source bounding box k_rect_remap_lds would stage for every 64 x 16 destination tile (row pitch rounded up
    to a dword, the right and lower taps included), 0 for a tile without a valid pixel: (tiles down, tiles across)."""
    m = np.asarray(rmap, np.uint32)
    h, w = m.shape
    out = np.zeros(((h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W), np.int64)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            t = m[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W]
            t = t[t != R.INVALID]
            if t.size:
                ix, iy = ((t & 0xFFFF) >> 5).astype(np.int64), (t >> 21).astype(np.int64)
                out[ty, tx] = ((ix.max() + 1 - ix.min() + 1 + 3) & ~3) * (iy.max() + 1 - iy.min() + 1)
    return out


class EdgeCase:
    """One row of the table below: a camera, the new intrinsics, the sizes, the layouts of the source and destination
    buffers, and (computed once, read-only) the restatement's map, the noise frames and the restatement's images."""

    def __init__(self, name, cam, new_K, src, dst, n_frames=EDGE_FRAMES, fill=FILL, tight=False, seed=0):
        self.name, self.cam, self.new_K, self.src, self.dst = name, cam, tuple(float(v) for v in new_K), src, dst
        self.n_frames, self.fill, self.seed = n_frames, fill, seed
        if tight:                                                # pitch = width: the aligned dword store on every row
            assert dst[0] % 4 == 0
            self.src_pitch, self.dst_pitch = src[0], dst[0]
            self.src_stride, self.dst_stride = src[0] * src[1], dst[0] * dst[1]
        else:                                                    # shape (b)'s pattern
            self.src_pitch, self.dst_pitch = src[0] + 16, (dst[0] + 5) | 1
            self.src_stride, self.dst_stride = self.src_pitch * src[1] + 96, self.dst_pitch * dst[1] + 37

    @functools.cached_property
    def map(self):
        m = R.build_map(self.cam, self.new_K, self.src[0], self.src[1], self.dst[0], self.dst[1])
        m.setflags(write=False)
        return m

    @functools.cached_property
    def forms(self):
        return read_forms(self.map, self.src[0])

    @functools.cached_property
    def frames(self):
        f = np.random.default_rng(100 + self.seed).integers(0, 256, (self.n_frames, self.src[1], self.src[0]), dtype=np.uint8)
        f.setflags(write=False)
        return f

    @functools.cached_property
    def want(self):
        out = R.remap(self.frames, self.map, self.fill)
        out.setflags(write=False)
        return out

    def src_buffer(self, frames=None):
        return padded(self.frames if frames is None else frames, self.src_pitch, self.src_stride)

    def images(self, buf, n=None):
        """(images, True when no padding byte differs from the 0x5A prefill) of a destination buffer of n frames."""
        n = self.n_frames if n is None else n
        img, is_pad = unpadded(buf, n, self.dst[1], self.dst[0], self.dst_pitch, self.dst_stride)
        return img, bool((np.asarray(buf, np.uint8).reshape(n, self.dst_stride)[is_pad] == 0x5A).all())


def _edge_cases():
    cal = R.scaled_calibration(96, 64, R.EUROC_MH)
    K, D = cal["K_l"], tuple(cal["D_l"]) + (0.01,)                # k3 != 0
    s96 = (96, 64)
    big = R.camera(K_L, D_L + (0.01,))
    cases = [
        EdgeCase("zoom45", R.camera(K, D), (0.45 * K[0], 0.45 * K[1], 30.25, 22.5), s96, (61, 45), seed=1),
        EdgeCase("zoom20", R.camera(K, D), (0.2 * K[0], 0.2 * K[1], 14.25, 10.5), s96, (29, 21), fill=255, seed=2),
        EdgeCase("roll20", R.camera(K, D, rot_z(20)), (0.8 * K[0], 0.8 * K[1], 46.25, 31.5), s96, (93, 63), seed=3),
        EdgeCase("roll90", R.camera(K, D, rot_z(90)), (K[0], K[1], 31.5, 47.25), s96, (64, 96), tight=True, seed=4),
        EdgeCase("yaw75", R.camera(K, D, rot_y(75)), (0.15 * K[0], 0.15 * K[1], 20.0, 16.0), s96, (41, 33), seed=5),
        EdgeCase("src8", R.camera((6.0, 6.0, 3.5, 3.5), (-0.1, 0.01, 0.001, 0.001, 0.0)), (3.0, 3.0, 5.25, 4.5), (8, 8), (11, 9),
                 seed=6),
        EdgeCase("src2", R.camera((2.0, 2.0, 0.5, 0.5)), (8.0, 8.0, 2.0, 1.0), (2, 2), (3, 1), seed=7),
        # the packing's limits: destination (u, v) looks at source (u + 0.5, v + 2023.5), so column 2045 and row 22 read the
        # last taps inside a 2047 x 2047 source (ix = iy = 2045, bit 31 of the word set) and column 2046 and row 23 leave it
        EdgeCase("limits", R.camera((1000.0, 1000.0, 1023.0, 1023.0)), (1000.0, 1000.0, 1022.5, -1000.5), (R.MAX_DIM, R.MAX_DIM),
                 (R.MAX_DIM, 24), n_frames=1, seed=8),
        # for the variants (tools/rect_check.py) only: tiles whose source box does and does not fit k_rect_remap_lds's LDS
        EdgeCase("zoom20_big", big, (0.2 * K_L[0], 0.2 * K_L[1], 80.25, 48.5), SIZE, (160, 96), n_frames=3, seed=9),
    ]
    return {c.name: c for c in cases}


EDGE_CASES = _edge_cases()
DEVICE_CASES = [n for n in EDGE_CASES if n != "zoom20_big"]      # test_gpu_rectify.py and the emulation
VARIANT_SETTINGS = [{}, {"ARIA_RECT_READ": "taps"}, {"ARIA_RECT_READ": "lds"}, {"ARIA_RECT_GROUP": "1"}, {"ARIA_RECT_GROUP": "3"}]


def form_counts(case):
    """What a case reaches, as DESIGN.md's table states it."""
    f = case.forms
    n = lambda a: int(np.count_nonzero(a))   # noqa: E731
    return dict(lanes=f["form"].size, none=n(f["form"] == NONE), rows=n(f["form"] == ROWS), taps=n(f["form"] == TAPS),
                xspan6=n(f["xspan"] == 6), xspan7=n(f["xspan"] == 7), xspan_max=int(f["xspan"].max()),
                yspan1=n(f["yspan"] == 1), yspan2=n(f["yspan"] == 2), yspan_max=int(f["yspan"].max()),
                edge_only=n(f["edge_only"]), mixed=n(f["mixed"]), mixed_rows=n(f["mixed"] & (f["form"] == ROWS)),
                low_pair=n((f["form"] == ROWS) & (f["yspan"] == 1)),
                last_row=n((f["form"] == ROWS) & (f["yspan"] == 0) & (f["y0"] == case.src[1] - 2)),
                invalid_share=float((case.map == R.INVALID).mean()))


# ---- points: non-finite and far keypoints, cameras that look away ---------------------------------------------------------
POINT_COUNTS = np.array([257, KP_STRIDE], np.int32)
POINT_HEAD = [(np.nan, 3.0), (np.inf, 3.0), (-np.inf, 3.0), (3e9, 3.0), (3.4e38, 3.0), (100.0, np.nan)]
POINT_NONFINITE = [0, 1, 2, 5]                                   # the records of POINT_HEAD with a NaN or an infinity


@functools.lru_cache(maxsize=None)
def point_cameras():
    """(name, camera) of the points cases; EuRoC's K at 752x480 with k3 = 0.01, new K = K."""
    d = D_L + (0.01,)
    return (("identity", R.camera(K_L, d)), ("yaw75", R.camera(K_L, d, rot_y(75))), ("yaw-100", R.camera(K_L, d, rot_y(-100))))


@functools.lru_cache(maxsize=None)
def edge_keypoints():
    """Two frames of KP_STRIDE records far around the image, each opening with POINT_HEAD; counts POINT_COUNTS."""
    rng = np.random.default_rng(22)
    k = np.zeros((2, KP_STRIDE), KP_DTYPE)
    k["x"] = rng.uniform(-2000, 3000, (2, KP_STRIDE)).astype(np.float32)
    k["y"] = rng.uniform(-1500, 2000, (2, KP_STRIDE)).astype(np.float32)
    for j, (x, y) in enumerate(POINT_HEAD):
        k["x"][:, j], k["y"][:, j] = np.float32(x), np.float32(y)
    k["size"] = rng.uniform(20, 80, (2, KP_STRIDE)).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, (2, KP_STRIDE)).astype(np.float32)
    k["response"] = rng.uniform(0, 1, (2, KP_STRIDE)).astype(np.float32)
    k["octave"] = rng.integers(0, 8, (2, KP_STRIDE))
    k.setflags(write=False)
    return k


def ref_edge_points(cam, kp, counts):
    """ref_points for a camera of point_cameras() (new K = its K)."""
    out = kp.copy()
    for f, n in enumerate(counts):
        if 0 <= n <= kp.shape[1]:
            out[f, :n] = R.undistort_points(kp[f, :n], cam, cam["K"])
    return out


@functools.lru_cache(maxsize=None)
def ref_edge_points_all():
    """name -> (the restatement's records, Z <= 0 per record of frame 0 up to its count)."""
    kp = edge_keypoints()
    out = {}
    for name, cam in point_cameras():
        want = ref_edge_points(cam, kp, POINT_COUNTS)
        want.setflags(write=False)
        n = POINT_COUNTS[0]
        with np.errstate(all="ignore"):
            Z = R.undistort_xy(kp[0, :n]["x"], kp[0, :n]["y"], cam, cam["K"])[2]
        out[name] = (want, Z <= 0)
    return out
