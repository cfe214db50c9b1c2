"""Postprocess cases of the object-detector stage, worked by hand: shared by tests/test_detect_host.py (the restatement) and
tests/test_gpu_detect.py (the same table through the device)."""
import os
import subprocess

import numpy as np

from aria_slam_amd import detect_ref as R


def _rows(*rows):
    return np.array(rows, np.float32).reshape(-1, 6)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")


def build_selftest():
    """Build tests/cpp/det_selftest.cpp against the adapters library; returns the executable."""
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    exe = os.path.join(ROOT, "build", "det_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "det_selftest.cpp")
    lib = os.path.join(PKG, "libaria_hip_adapters.so")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(lib)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(PKG, "host", "include"), src, "-o", exe, "-L" + PKG, "-laria_hip_adapters",
                               "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    return exe


NAN = float("nan")
# name -> (raw rows, kwargs, expected [(x1, y1, x2, y2, class)] in output order, expected number of dynamic boxes)
POST_CASES = {
    "empty_frame": (np.zeros((0, 6), np.float32), {}, [], 0),
    "all_below_threshold": (_rows([0, 0, 10, 10, 0.3, 0], [5, 5, 9, 9, 0.49, 0]), {}, [], 0),
    # conf_i == conf passes TRTInference.cpp:116 (>=) and falls at NMSBoxes' strict score > threshold
    "score_equal_to_conf": (_rows([0, 0, 10, 10, 0.5, 0], [20, 20, 30, 30, 0.75, 0]), {}, [(20, 20, 30, 30, 0)], 1),
    "two_identical_boxes": (_rows([0, 0, 10, 10, 0.9, 0], [0, 0, 10, 10, 0.8, 0]), {}, [(0, 0, 10, 10, 0)], 1),
    # sharing an edge: intersection width 0 -> empty -> overlap 0
    "edge_touching_boxes": (_rows([0, 0, 10, 10, 0.9, 0], [10, 0, 20, 10, 0.8, 0]), {}, [(0, 0, 10, 10, 0), (10, 0, 20, 10, 0)], 2),
    # A = [0, 10), B = [4, 14), C = [8, 18) on x, height 10. IoU(A, B) = 60 / 140 = 0.43 > 0.4, IoU(B, C) the same,
    # IoU(A, C) = 20 / 180 = 0.11: A suppresses B, B would suppress C but is gone, A does not -> C survives
    "chain_a_b_c": (_rows([0, 0, 10, 10, 0.9, 1], [4, 0, 14, 10, 0.8, 1], [8, 0, 18, 10, 0.7, 1]), {"nms": 0.4},
                    [(0, 0, 10, 10, 1), (8, 0, 18, 10, 1)], 2),
    # equal scores keep candidate order (stable sort); the disjoint third sorts first
    "equal_scores_index_order": (_rows([30, 0, 40, 10, 0.8, 2], [0, 0, 10, 10, 0.8, 3], [60, 0, 70, 10, 0.9, 5], [0, 0, 10, 10, 0.8, 7]), {},
                                 [(60, 0, 70, 10, 5), (30, 0, 40, 10, 2), (0, 0, 10, 10, 3)], 3),
    # Aa + Ab = 0 <= DBL_EPSILON -> jaccardDistance 0 -> overlap 1 > nms, although the two do not even touch
    "two_zero_area_boxes": (_rows([5, 5, 5, 9, 0.9, 0], [50, 50, 58, 50, 0.8, 0]), {}, [(5, 5, 5, 9, 0)], 1),
    "zero_area_and_a_real_box": (_rows([5, 5, 5, 9, 0.9, 0], [0, 0, 10, 10, 0.8, 0]), {}, [(5, 5, 5, 9, 0), (0, 0, 10, 10, 0)], 2),
    # (int) truncates toward zero: -3.7 -> -3, -0.9 -> 0, 5.99 -> 5
    "negative_coordinates": (_rows([-3.7, -0.9, 5.99, 7.5, 0.9, 16]), {}, [(-3, 0, 5, 7, 16)], 1),
    "nan_score": (_rows([0, 0, 10, 10, NAN, 0], [20, 20, 30, 30, 0.9, 4]), {}, [(20, 20, 30, 30, 4)], 0),
    "nan_and_inf_coordinates": (_rows([NAN, 0, 10, 10, 0.9, 0], [0, 0, float("inf"), 10, 0.9, 0], [1, 1, 4, 4, 0.6, 0]), {}, [(1, 1, 4, 4, 0)], 1),
    # 2^21 is outside +-2^20 (dropped); 2^20 itself is inside
    "coordinate_2_pow_21": (_rows([0, 0, 2.0 ** 21, 10, 0.9, 0], [0, 0, 2.0 ** 20, 10, 0.8, 0]), {}, [(0, 0, 2 ** 20, 10, 0)], 1),
    # scale: 1280 x 320 source on a 640 x 640 input -> x doubles, y halves, in fp32, then truncation
    "scaled": (_rows([10.3, 10.3, 20.7, 21.9, 0.9, 0]), {"src_w": 1280, "src_h": 320}, [(20, 5, 41, 10, 0)], 1),
    "dynamic_subset": (_rows([0, 0, 10, 10, 0.9, 4], [20, 0, 30, 10, 0.8, 0], [40, 0, 50, 10, 0.7, 8], [60, 0, 70, 10, 0.6, 16]), {},
                       [(0, 0, 10, 10, 4), (20, 0, 30, 10, 0), (40, 0, 50, 10, 8), (60, 0, 70, 10, 16)], 2),
    "dynamic_all": (_rows([0, 0, 10, 10, 0.9, 4], [20, 0, 30, 10, 0.8, 0], [40, 0, 50, 10, 0.7, 8]), {"dynamic_classes": R.ALL_CLASSES},
                    [(0, 0, 10, 10, 4), (20, 0, 30, 10, 0), (40, 0, 50, 10, 8)], 3),
    "dynamic_custom": (_rows([0, 0, 10, 10, 0.9, 4], [20, 0, 30, 10, 0.8, 0], [40, 0, 50, 10, 0.7, 8]), {"dynamic_classes": (8, 4)},
                       [(0, 0, 10, 10, 4), (20, 0, 30, 10, 0), (40, 0, 50, 10, 8)], 2),
    # class_id = (int)raw[5]: truncation; a NaN gives 0
    "class_cast": (_rows([0, 0, 10, 10, 0.9, 2.9], [20, 0, 30, 10, 0.8, NAN], [40, 0, 50, 10, 0.7, -1.5]), {},
                   [(0, 0, 10, 10, 2), (20, 0, 30, 10, 0), (40, 0, 50, 10, -1)], 2),
}


def run_case_ref(name):
    raw, kw, _, _ = POST_CASES[name]
    kw = dict(kw)
    return R.postprocess_ref(raw, kw.pop("src_w", 640), kw.pop("src_h", 640), 640, 640, **kw)


# ---- generated frames (n rows of [x1, y1, x2, y2, confidence, class_id], 640 x 640 network input, scale 1)
def disjoint_frame(n=300, seed=5):
    """n 10 x 10 boxes on a 12-pixel grid: nothing overlaps, every box is kept, the output order is the pure sort. The
    scores come from 40 values, so ties (index order) are everywhere."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    x, y = (i % 50) * 12.0, (i // 50) * 12.0
    sc = 0.55 + rng.integers(0, 40, n) / 100.0
    return np.stack([x, y, x + 10, y + 10, sc, rng.integers(0, 20, n)], 1).astype(np.float32)


def nested_frame(n=300):
    """A 600 x 600 box with the highest score and n - 1 boxes that differ from it by a few pixels: one is kept."""
    i = np.arange(n)
    raw = np.stack([i % 5, i % 7, 600 - i % 3, 600 - i % 4, 0.9 - i * 0.001, i % 20], 1).astype(np.float32)
    raw[0] = (0, 0, 600, 600, 0.95, 0)
    return raw


def random_frame(n=300, seed=7, canvas=64):
    """Integer boxes over a canvas x canvas area, sides 1..canvas/2, scores in sixteenths: heavy overlap, many ties, a few
    below the threshold."""
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, canvas, n), rng.integers(0, canvas, n)
    w, h = rng.integers(1, canvas // 2 + 1, n), rng.integers(1, canvas // 2 + 1, n)
    sc = rng.integers(6, 16, n) / 16.0
    return np.stack([x, y, x + w, y + h, sc, rng.integers(0, 20, n)], 1).astype(np.float32)


def iou_pairs_frame():
    """Pairs of 100 x 100 boxes shifted by s pixels along x, IoU = (100 - s) / (100 + s): s = 38 gives 62 / 138 = 0.4493
    (<= 0.45, both kept), s = 37 gives 63 / 137 = 0.4599 (suppressed). The same along y. Pairs are 200 pixels apart."""
    rows = []
    for k, (dx, dy) in enumerate(((38, 0), (37, 0), (0, 38), (0, 37))):
        x, y = (k % 2) * 300.0, (k // 2) * 300.0
        rows.append([x, y, x + 100, y + 100, 0.9 - 0.01 * k, 0])
        rows.append([x + dx, y + dy, x + dx + 100, y + dy + 100, 0.8 - 0.01 * k, 0])
    return np.array(rows, np.float32)


IOU_PAIRS_KEPT = [0, 2, 4, 6, 1, 5]      # candidate indices in output order: the four first boxes, then the s = 38 seconds
