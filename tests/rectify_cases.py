"""Shared inputs of the rectification tests (test_rectify_host.py, test_rectify_kernel_emulation.py, test_gpu_rectify.py,
test_cpp_rectify.py): the EuRoC MH cam0 / cam1 calibration as their sensor.yaml files state it, the shapes (a)-(d) the
device tests and the kernel emulation both run, and the restatement's results on them, computed once per process."""
import functools

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
