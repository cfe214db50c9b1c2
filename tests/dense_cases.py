"""Shared inputs of the dense stereo tests (test_dense_host.py, test_gpu_dense.py, test_cpp_dense.py): the shapes (a)-(f) the
device tests run and the restatement's results on them (aria_slam_amd/dense_ref.py), computed once per process and handed
out read-only."""
import functools

import numpy as np

from aria_slam_amd import dense_ref as R
from aria_slam_amd._lib import KP_DTYPE

K, BASELINE = R.EUROC_K, 0.110

# shape (a): the synthetic rectified scene (row disparities 7.0, 19.5, 42.25)
SCENE = (200, 96)
SCENE_SEEDS = (1, 2)
ACCURACY_SHAPES = ((200, 96), (320, 240))
# shape (b): W no multiple of 4, padded input and output layouts
NOISE = (131, 37)
IMG_PITCH, IMG_STRIDE = 160, 160 * 37 + 96
DISP_PITCH, DISP_STRIDE = 133, 133 * 37 + 11             # odd pitch: unaligned rows
DEPTH_PITCH, DEPTH_STRIDE = 140, 140 * 37 + 5
# shape (c): W < D, and a constant pair
NARROW = (40, 20)
CONST = (70, 9)
# shape (d): five pairs of shape (b)'s size
N_BATCH = 5
# shape (e)
PARAM_SETS = (dict(P1=1, P2=127), dict(uniqueness=0), dict(lr_max_diff=-1), dict(lr_max_diff=0))
# shape (f)
KP_STRIDE = 64
SAMPLE_COUNTS = (0, 1, KP_STRIDE)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def scene_pair(seed, W, H):
    left, right, d = R.stereo_pair(seed, W, H)
    return _ro(left, right, d)


@functools.lru_cache(maxsize=None)
def noise_pair(seed, W=NOISE[0], H=NOISE[1]):
    """Uniform noise on the left. The upper half of the right image is the left one moved by 9 px (valid disparities), the
    lower half is independent noise (ties between costs, uniqueness and left-right failures)."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right[:H // 2, :W - 9] = left[:H // 2, 9:]
    return _ro(left, right)


@functools.lru_cache(maxsize=None)
def const_pair(W=CONST[0], H=CONST[1]):
    a = np.full((H, W), 100, np.uint8)
    return _ro(a, a.copy())


@functools.lru_cache(maxsize=None)
def batch_pairs():
    """Shape (d): noise and scene pairs in turn, all 131x37."""
    W, H = NOISE
    out = [noise_pair(7), scene_pair(1, W, H)[:2], noise_pair(8), scene_pair(2, W, H)[:2], noise_pair(9)]
    return tuple((p[0], p[1]) for p in out)


_cache = {}


def ref(left, right, **cfg):
    """(d16, depth) of the restatement for a pair handed out by this module; one computation per pair and parameter set."""
    key = (id(left), id(right), tuple(sorted(cfg.items())))
    if key not in _cache:
        d16 = R.dense_disparity(left, right, **cfg)
        _cache[key] = (left, right) + _ro(d16, R.depth_map(d16, K, BASELINE))     # the pair is kept alive: ids stay unique
    return _cache[key][2:]


def padded_images(imgs, pitch, stride, fill=0xA5):
    """n images (H, W) laid out with `pitch` bytes per row and `stride` bytes per image, padding = fill."""
    n, (H, W) = len(imgs), imgs[0].shape
    buf = np.full((n, stride), fill, np.uint8)
    for k, im in enumerate(imgs):
        buf[k, :pitch * H].reshape(H, pitch)[:, :W] = im
    return buf


def unpadded(buf, n, H, W, pitch, stride):
    """(values (n, H, W), mask (n, stride) that is True on padding elements) of a pitched, strided output buffer."""
    buf = buf.reshape(n, stride)
    vals = buf[:, :pitch * H].reshape(n, H, pitch)[:, :, :W].copy()
    is_pad = np.ones((n, stride), bool)
    is_pad[:, :pitch * H].reshape(n, H, pitch)[:, :, :W] = False
    return vals, is_pad


@functools.lru_cache(maxsize=None)
def sample_keypoints():
    """Shape (f): (kp [3, KP_STRIDE], counts) on 131x37 maps. Coordinates reach two pixels outside the image on every side;
    a few sit exactly on .5 (round-half-even), one is NaN and one is huge."""
    W, H = NOISE
    rng = np.random.default_rng(31)
    kp = np.zeros((3, KP_STRIDE), KP_DTYPE)
    kp["x"] = rng.uniform(-2.4, W + 1.4, kp.shape).astype(np.float32)
    kp["y"] = rng.uniform(-2.4, H + 1.4, kp.shape).astype(np.float32)
    kp["size"], kp["angle"], kp["response"], kp["octave"] = 31.0, 10.0, 20.0, 0
    for f in range(3):
        kp["x"][f, :6] = [2.5, 3.5, -0.5, W - 0.5, W - 1.5, 20.25]
        kp["y"][f, :6] = [0.5, 1.5, 4.0, 5.0, H - 0.5, -0.5]
        kp["x"][f, 6], kp["y"][f, 6] = np.nan, 3.0
        kp["x"][f, 7], kp["y"][f, 7] = 3.0e9, 3.0
        kp["x"][f, 8:20] = rng.integers(12, W - 12, 12) + 0.25                 # inside, many on valid pixels
        kp["y"][f, 8:20] = rng.integers(1, H // 2 - 1, 12) - 0.25
    return _ro(kp), np.array(SAMPLE_COUNTS, np.int32)
