"""NumPy restatement of the object-detector stage around the network (include/aria_orb_hip.h, "object detector"): the
definition the kernels of csrc/detect_stage.hip are held to, bit for bit.

What it restates is the reference's host code around its TensorRT engine: TRTInference::preprocess
(src/legacy/TRTInference.cpp:68-93: cv::resize, BGR2RGB, /255, HWC -> CHW) and TRTInference::postprocess (:95-142: decode of
the [300, 6] head, scale, cast to int, threshold, cv::dnn::NMSBoxes), with the dynamic-class set of src/main.cpp:29-40. The
network between the two is not restated: it is whatever the caller injects.

OpenCV is not available where this was written and parity with it is not pinned. Every rule written from memory of OpenCV
4.9.0 is marked [RECALL] below; where this file and OpenCV disagree, this file is what the kernels compute.

Everything here is integer arithmetic, single correctly rounded fp32 / fp64 operations and copies, so the device is compared
bitwise and there is no tolerance anywhere.

Divergences from the reference, both replacing undefined behaviour:
  D1  A candidate with a non-finite coordinate, or a scaled coordinate outside +-2^20, is dropped before NMS. The reference
      casts such a float to int, which C++ leaves undefined.
  D2  Box areas are exact (int64). cv::Rect::area() is an int product and overflows for boxes the +-2^20 rule still admits.
One further definition where the reference is undefined: class_id = (int)raw[5] saturates at the int32 range and is 0 for a
NaN (what the device's conversion instruction gives)."""
import numpy as np

# src/main.cpp:29-40: person, bicycle, car, motorcycle, bus, train, truck, bird, cat, dog
DYNAMIC_CLASSES = (0, 1, 2, 3, 5, 6, 7, 14, 15, 16)
ALL_CLASSES = "all"

# byte-for-byte aria::core::Detection (reference include/core/Types.hpp:103-112), 24 bytes; and aria_box, 16 bytes
DETECTION_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("confidence", "<f4"), ("class_id", "<i4")])
BOX_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS          # INTER_RESIZE_COEF_SCALE = 2048 [RECALL]
COORD_LIMIT = float(1 << 20)       # D1
MAX_CANDIDATES = 1024
F32 = np.float32


def resize_table(src, dst):
    """Per destination index along one axis: (offset of the first tap, offset of the second tap, weight of the second tap in
    1/2048). [RECALL] cv::resize's 8-bit INTER_LINEAR path (resizeGeneric_ with HResizeLinear / VResizeLinear): in fp32,
    f = (d + 0.5f) * (src / (float)dst) - 0.5f, s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1,
    f = 0 and the second tap is the last pixel again; the weights are cvRound(f * 2048) (half to even) and 2048 minus it,
    held as 16-bit values."""
    d = np.arange(dst, dtype=F32)
    scale = F32(src) / F32(dst)
    f = (d + F32(0.5)) * scale - F32(0.5)
    assert f.dtype == F32
    s = np.floor(f)
    frac = f - s
    s = s.astype(np.int64)
    left, right = s < 0, s >= src - 1
    s = np.where(left, 0, np.where(right, src - 1, s))
    frac = np.where(left | right, F32(0), frac).astype(F32)
    a1 = np.rint(frac * F32(COEF_ONE)).astype(np.int32)
    s1 = np.minimum(s + 1, src - 1)
    return s.astype(np.int32), s1.astype(np.int32), a1


def resize_linear_u8(img, out_w, out_h):
    """(H, W) or (H, W, C) uint8 -> (out_h, out_w[, C]) uint8. [RECALL] the fixed-point arithmetic of the 8-bit path: the
    horizontal pass S = p0 * (2048 - a) + p1 * a in int32, the vertical pass
    (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    H, W = img.shape[:2]
    x0, x1, ax = resize_table(W, out_w)
    y0, y1, ay = resize_table(H, out_h)
    src = img.astype(np.int32)
    sh = (1, out_w) + (1,) * (img.ndim - 2)
    a1 = ax.reshape(sh)
    hpass = src[:, x0] * (COEF_ONE - a1) + src[:, x1] * a1                 # (H, out_w[, C]) int32
    b1 = ay.reshape((out_h,) + (1,) * (img.ndim - 1))
    b0 = COEF_ONE - b1
    v = (((b0 * (hpass[y0] >> 4)) >> 16) + ((b1 * (hpass[y1] >> 4)) >> 16) + 2) >> 2
    assert v.min(initial=0) >= 0 and v.max(initial=0) <= 255
    return v.astype(np.uint8)


def preprocess_ref(images, in_w, in_h, channels=None, swap_rb=True, half=False):
    """TRTInference::preprocess (src/legacy/TRTInference.cpp:68-93) for a batch. images: uint8 (B, H, W) or (B, H, W, 3);
    returns (B, 3, in_h, in_w) float32, or float16 with half.
      resize     resize_linear_u8 (cv::resize(image, resized, Size(input_w, input_h)), :71: a stretch, no letterbox)
      scale      float32(v) * float32(1.0 / 255.0) (convertTo(CV_32FC3, 1.0f / 255.0f), :76) [RECALL: convertTo's 8u -> 32f
                 with a scale is one fp32 multiply]
      planes     HWC -> CHW (:79-87); swap_rb exchanges planes 0 and 2 (cvtColor BGR2RGB, :75)
      gray       channels == 1: the plane three times, what cvtColor GRAY2BGR in front of detect() gives
                 (src/euroc_eval.cpp:149)
      half       the fp32 product rounded to float16 once, to nearest even"""
    images = np.asarray(images)
    assert images.dtype == np.uint8 and images.ndim in (3, 4)
    c = 1 if images.ndim == 3 else images.shape[3]
    if channels is not None:
        assert channels == c
    assert c in (1, 3)
    B = images.shape[0]
    out = np.empty((B, 3, in_h, in_w), np.float32)
    k = F32(1.0 / 255.0)
    for b in range(B):
        r = resize_linear_u8(images[b], in_w, in_h).astype(np.float32) * k
        if c == 1:
            out[b, :] = r[None]
        else:
            planes = np.transpose(r, (2, 0, 1))
            out[b] = planes[::-1] if swap_rb else planes
    return out.astype(np.float16) if half else out


def _trunc_int(v):
    """(int)float for values already known to lie inside +-2^20: truncation toward zero."""
    return np.trunc(v).astype(np.int64)


def _class_id(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.where(np.isnan(v), F32(0), v).astype(np.float64))
    return np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32)


def rect_overlap(a, b):
    """1.f - (float)jaccardDistance(a, b) of cv::dnn::NMSBoxes on two integer boxes (x1, y1, x2, y2) [RECALL]:
    Rect = (x1, y1, x2 - x1, y2 - y1); area = w * h whatever the signs (exact here, D2); a & b is empty (area 0) when its
    width or height is <= 0; jaccardDistance = 0 when Aa + Ab <= DBL_EPSILON, else 1 - Aab / (Aa + Ab - Aab) in fp64."""
    ax1, ay1, ax2, ay2 = (int(v) for v in a)
    bx1, by1, bx2, by2 = (int(v) for v in b)
    Aa = np.float64((ax2 - ax1) * (ay2 - ay1))
    Ab = np.float64((bx2 - bx1) * (by2 - by1))
    if Aa + Ab <= np.finfo(np.float64).eps:
        jd = np.float64(0.0)
    else:
        ix, iy = max(ax1, bx1), max(ay1, by1)
        iw, ih = min(ax2, bx2) - ix, min(ay2, by2) - iy
        Aab = np.float64(0.0) if (iw <= 0 or ih <= 0) else np.float64(iw * ih)
        with np.errstate(divide="ignore", invalid="ignore"):
            jd = np.float64(1.0) - Aab / (Aa + Ab - Aab)
    return F32(1.0) - F32(jd)


def postprocess_ref(raw, src_w, src_h, in_w, in_h, conf=0.5, nms=0.45, dynamic_classes=None):
    """TRTInference::postprocess (src/legacy/TRTInference.cpp:95-142) for one frame. raw: (n_cand, 6) float32 rows
    [x1, y1, x2, y2, confidence, class_id] in network-input coordinates, n_cand <= 1024. Returns (detections, boxes):
    DETECTION_DTYPE records in NMSBoxes' output order, and BOX_DTYPE records of those whose class is in dynamic_classes
    (None: src/main.cpp:29-40; ALL_CLASSES: every class), same order.
      scale      scale_x = (float)src_w / in_w, scale_y likewise (:164-165)
      threshold  confidence >= conf (:116); a NaN fails
      cast       bx = (int)(x * scale): the fp32 product truncated toward zero (:118-121); D1 drops what the cast cannot hold
      NMSBoxes   [RECALL] score > conf (strict); std::stable_sort by descending score, so ties keep candidate order; greedy in
                 that order: a box is kept when rect_overlap(box, k) <= nms for every box k kept before it. A suppressed box
                 suppresses nothing.
      output     x1, y1, x2, y2 = (float)bx1, by1, bx2, by2 -- the corners mode 0 of aria_flag_keypoints_device expects"""
    raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 6)
    assert len(raw) <= MAX_CANDIDATES
    conf, nms = F32(conf), F32(nms)
    sx, sy = F32(src_w) / F32(in_w), F32(src_h) / F32(in_h)
    with np.errstate(invalid="ignore", over="ignore"):
        p = raw[:, :4] * np.array([sx, sy, sx, sy], F32)
        assert p.dtype == F32
        ok = (raw[:, 4] >= conf) & (raw[:, 4] > conf)
        ok &= np.isfinite(raw[:, :4]).all(axis=1) & (np.abs(p) <= F32(COORD_LIMIT)).all(axis=1)
    idx = np.nonzero(ok)[0]
    order = idx[np.argsort(-raw[idx, 4].astype(np.float64), kind="stable")]
    box = _trunc_int(np.where(ok[:, None], p, F32(0)))
    cls = _class_id(raw[:, 5])
    kept = []
    for i in order:
        if all(rect_overlap(box[i], box[k]) <= nms for k in kept):
            kept.append(i)
    dets = np.zeros(len(kept), DETECTION_DTYPE)
    for n, i in enumerate(kept):
        dets[n] = (F32(box[i, 0]), F32(box[i, 1]), F32(box[i, 2]), F32(box[i, 3]), raw[i, 4], cls[i])
    if isinstance(dynamic_classes, str):
        assert dynamic_classes == ALL_CLASSES
        dyn = np.ones(len(dets), bool)
    else:
        ids = DYNAMIC_CLASSES if dynamic_classes is None else tuple(int(c) for c in dynamic_classes)
        dyn = np.isin(dets["class_id"], np.array(ids, np.int32).reshape(-1))
    boxes = np.zeros(int(dyn.sum()), BOX_DTYPE)
    for k in ("x1", "y1", "x2", "y2"):
        boxes[k] = dets[k][dyn]
    return dets, boxes


def postprocess_batch_ref(raw, src_w, src_h, in_w, in_h, conf=0.5, nms=0.45, dynamic_classes=None):
    """postprocess_ref per frame of a (B, n_cand, 6) array: [(detections, boxes)] * B."""
    raw = np.asarray(raw, np.float32)
    return [postprocess_ref(raw[b], src_w, src_h, in_w, in_h, conf, nms, dynamic_classes) for b in range(raw.shape[0])]
