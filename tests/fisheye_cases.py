"""Shared inputs of the fisheye (KB4) tests (test_fisheye_host.py, test_fisheye_kernel_emulation.py, test_gpu_fisheye.py,
test_cpp_fisheye.py): the cameras, four map / remap cases and a paraxial fifth with the layouts of rectify_cases.EdgeCase,
the points cases with rectify_cases.edge_keypoints' record layout, and the restatement's results on all of them, computed once per process."""
import functools

import numpy as np

import rectify_cases as RC
from rectify_cases import EdgeCase, padded, read_forms, rot_y, unpadded   # noqa: F401  (the tests take them from here)
from aria_slam_amd import rectify_ref as R
from aria_slam_amd._lib import KP_DTYPE

SRC = (96, 64)
K_A, D_A = (36.0, 36.2, 47.3, 31.6), (-0.027, 0.101, -0.071, 0.0125)
K_FOLD, D_FOLD = (36.0, 36.0, 47.5, 31.5), (-0.2, 0.0, 0.0, 0.0)              # D(a) = 1 - 0.6 a^2 vanishes at 1.291 rad
K_WIDE, D_WIDE = (190.978, 190.973, 254.931, 256.897), (0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673)
WIDE_SIZE = (512, 512)
WIDE_NEW_KS = (K_WIDE, (60.0, 60.0, 255.5, 255.5))                            # host tests only
A = R.camera(K_A, D_A, model="kb4")
FOLD = R.camera(K_FOLD, D_FOLD, model="kb4")
WIDE512 = R.camera(K_WIDE, D_WIDE, model="kb4")
# a 96x64 crop behind a long lens, all k zero: the whole image is paraxial, the camera is a pinhole to 3e-6 px
K_TELE = (2.0e5, 2.02e5, 47.3, 31.6)
TELE_NEW_K = (0.93 * K_TELE[0], 0.93 * K_TELE[1], 46.85, 31.15)               # every fraction of a pixel occurs
TELE = R.camera(K_TELE, (0.0,) * 4, model="kb4")
N_FRAMES = 9                                                                  # frame groups of 8 and 1

# the rig: the EuRoC T_BS pair with camera A on both sides, at 96x64
RIG = dict(K_l=K_A, K_r=K_A, D_l=D_A, D_r=D_A, T_BS_l=RC.T_BS_L, T_BS_r=RC.T_BS_R, size=SRC, model="kb4")
RIG_DST = (96, 64)


def _cases():
    cl, _, nk, _ = R.rectified_cameras(RIG)
    cases = [
        EdgeCase("zoom10", A, (10.0, 10.0, 30.25, 22.5), SRC, (61, 45), n_frames=N_FRAMES, seed=21),
        EdgeCase("fold8", FOLD, (8.0, 8.0, 30.25, 22.5), SRC, (61, 45), n_frames=N_FRAMES, seed=22),
        EdgeCase("yaw75", R.camera(K_A, D_A, rot_y(75), "kb4"), (6.0, 6.0, 20.0, 16.0), SRC, (41, 33), n_frames=N_FRAMES, seed=23),
        EdgeCase("rig", cl, nk, SRC, RIG_DST, n_frames=N_FRAMES, seed=24),      # the left camera of the rig
        EdgeCase("tele", TELE, TELE_NEW_K, SRC, SRC, n_frames=N_FRAMES, seed=25),  # rect_atan(r) / r at r below 4e-4
    ]
    return {c.name: c for c in cases}


CASES = _cases()
# invalid share of each map as the prototype measured it (asserted within 0.03 by test_fisheye_host.py)
INVALID_SHARE = {"zoom10": 0.237, "fold8": 0.198, "yaw75": 0.616}

# ---- points ---------------------------------------------------------------------------------------------------------------
KP_STRIDE = RC.KP_STRIDE
POINT_COUNTS = RC.POINT_COUNTS                                                # (257, 300)


def point_cameras():
    """(name, camera) of the points cases; new K = the camera's K."""
    return (("A", A), ("FOLD", FOLD), ("A_yaw75", R.camera(K_A, D_A, rot_y(75), "kb4")))


@functools.lru_cache(maxsize=None)
def keypoints():
    """Two frames of KP_STRIDE records uniform in [-0.5 W, 1.5 W] x [-0.5 H, 1.5 H], each opening with the six records of
    rectify_cases.POINT_HEAD (NaN, infinities, huge values)."""
    rng = np.random.default_rng(31)
    k = np.zeros((2, KP_STRIDE), KP_DTYPE)
    k["x"] = rng.uniform(-0.5 * SRC[0], 1.5 * SRC[0], (2, KP_STRIDE)).astype(np.float32)
    k["y"] = rng.uniform(-0.5 * SRC[1], 1.5 * SRC[1], (2, KP_STRIDE)).astype(np.float32)
    for j, (x, y) in enumerate(RC.POINT_HEAD):
        k["x"][:, j], k["y"][:, j] = np.float32(x), np.float32(y)
    k["size"] = rng.uniform(20, 80, (2, KP_STRIDE)).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, (2, KP_STRIDE)).astype(np.float32)
    k["response"] = rng.uniform(0, 1, (2, KP_STRIDE)).astype(np.float32)
    k["octave"] = rng.integers(0, 8, (2, KP_STRIDE))
    k.setflags(write=False)
    return k


def ref_points(cam, kp, counts):
    """The restatement of step 4k on (frames, stride) records (new K = the camera's K): records at and beyond a frame's count,
    and frames whose count is out of range, stay as they are."""
    out = kp.copy()
    for f, n in enumerate(counts):
        if 0 <= n <= kp.shape[1]:
            out[f, :n] = R.undistort_points(kp[f, :n], cam, cam["K"])
    return out


@functools.lru_cache(maxsize=None)
def ref_points_all():
    """name -> the restatement's records of keypoints() with POINT_COUNTS."""
    out = {}
    for name, cam in point_cameras():
        want = ref_points(cam, keypoints(), POINT_COUNTS)
        want.setflags(write=False)
        out[name] = want
    return out


def write_sensor_yaml(path, K, D, T_BS, size, model="equidistant"):
    """rectify_cases.write_sensor_yaml with another distortion_model line."""
    RC.write_sensor_yaml(path, K, D, T_BS, size)
    text = open(path).read()
    assert "distortion_model: radial-tangential\n" in text
    with open(path, "w") as f:
        f.write(text.replace("distortion_model: radial-tangential\n", "distortion_model: %s\n" % model))
