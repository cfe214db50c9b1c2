"""NumPy restatement of the rectification stage (include/aria_orb_hip.h, "rectification"; kernels in csrc/rectify.hip).
The reference parses the radtan coefficients of cam0/sensor.yaml and never uses them, and has no stereo rectification, so
this file IS the definition: the device is held to it bit for bit. Every fp64 step below uses only + - * / and sqrt in the
header's order with every sum taken left to right (no contraction); the pixel step is integer.

Parity with OpenCV's stereoRectify / initUndistortRectifyMap / remap (and its fisheye:: functions) is not pinned and not
claimed. Two models: radtan (k1, k2, p1, p2, k3) and the fisheye model KB4 (Kannala-Brandt k1..k4: OpenCV's "fisheye",
Kalibr's "equidistant"), the header's steps 2k and 4k. KB4 needs atan and tan; rect_atan and rect_tan below build them from
+ - * / and sqrt alone, so the bitwise rule holds for KB4 as it does for radtan. Out of scope: Aria's FISHEYE624 (its 12
coefficients do not fit the camera record), KB3, rays at or beyond 90 degrees from the axis (a pinhole destination cannot
hold them), cylindrical and equirectangular destinations.

Also raw_stereo_pair, the synthetic raw (distorted, rotated) pair of the tests and tools."""
import math

import numpy as np

from ._lib import KP_DTYPE

# EuRoC MH cam0: the defaults of aria_rect_default_config
EUROC_K = (458.654, 457.296, 367.215, 248.375)
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)
# The EuRoC MH rig as its two sensor.yaml files state it: the synthetic raw pairs of the tests and tools use it
EUROC_MH = dict(
    K_l=EUROC_K, D_l=EUROC_D[:4], K_r=(457.587, 456.134, 379.999, 255.238),
    D_r=(-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05),
    T_BS_l=(0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975,
            0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768,
            -0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949, 0.0, 0.0, 0.0, 1.0),
    T_BS_r=(0.0125552670891, -0.999755099723, 0.0182237714554, -0.0198435579556,
            0.999598781151, 0.0130119051815, 0.0251588363115, 0.0453689425024,
            -0.0253898008918, 0.0179005838253, 0.999517347078, 0.00786212447038, 0.0, 0.0, 0.0, 1.0),
    size=(752, 480))
INVALID = 0xFFFFFFFF
MAX_DIM = 2047
POINT_ITERATIONS = 20
FISHEYE_POINT_ITERATIONS = 10                                   # Newton steps of step 4k (OpenCV's count)
FISHEYE_RESIDUAL = 1e-9                                         # |a P(a) - td| of a Newton run that converged
HALF_PI = 1.5707963267948966
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
MODELS = ("radtan", "kb4")                                      # ARIA_RECT_MODEL_RADTAN = 0, ARIA_RECT_MODEL_KB4 = 1
MODEL_NAMES = {"radtan": "radtan", "radial-tangential": "radtan", "plumb_bob": "radtan",
               "kb4": "kb4", "equidistant": "kb4", "fisheye": "kb4"}


def camera(K, dist=(), R=IDENTITY, model="radtan"):
    """A camera as the stage takes it: dict(K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3), R = 9 row-major). With
    model = "kb4" dist is exactly (k1, k2, k3, k4), stored as (k1, k2, k3, k4, 0.0), and the dict says model = "kb4"; a
    radtan dict carries no model key."""
    d = [float(v) for v in np.asarray(dist, np.float64).reshape(-1)]
    out = dict(K=tuple(float(v) for v in K), dist=tuple(d + [0.0] * (5 - len(d))),
               R=tuple(float(v) for v in np.asarray(R, np.float64).reshape(9)))
    if model == "kb4":
        if len(d) != 4:
            raise ValueError("kb4 takes exactly k1, k2, k3, k4")
        out["model"] = "kb4"
    elif model != "radtan":
        raise ValueError("model %r is neither 'radtan' nor 'kb4'" % (model,))
    elif len(d) > 5:
        raise ValueError("radtan takes k1, k2, p1, p2 and an optional k3")
    return out


def model_of(cam):
    """"radtan" or "kb4": the model key of a camera dict (absent = radtan)."""
    m = cam.get("model", "radtan")
    if m not in MODELS:
        raise ValueError("model %r is neither 'radtan' nor 'kb4'" % (m,))
    return m


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def stereo_geometry(K_l, K_r, T_BS_l, T_BS_r, new_K=None):
    """Step 1 in Python floats (IEEE fp64, one rounding per operation). T_BS: 4x4 sensor-to-body. new_K: (fx', fy', cx',
    cy') with zeros = the default of that entry. Returns dict(R1, R2 (3x3), R, t (x_r = R x_l + t), new_K, baseline).
    R is T's rotation block after one Gram-Schmidt pass over its rows."""
    A = [[float(v) for v in row] for row in np.asarray(T_BS_l, np.float64).reshape(4, 4)]
    B = [[float(v) for v in row] for row in np.asarray(T_BS_r, np.float64).reshape(4, 4)]
    # inverse_rigid(T_BS_r) = [Rr^T | -(Rr^T tr)]
    inv = [[B[0][i], B[1][i], B[2][i], -(B[0][i] * B[0][3] + B[1][i] * B[1][3] + B[2][i] * B[2][3])] for i in range(3)]
    R = [[inv[i][0] * A[0][j] + inv[i][1] * A[1][j] + inv[i][2] * A[2][j] for j in range(3)] for i in range(3)]
    t = [inv[i][0] * A[0][3] + inv[i][1] * A[1][3] + inv[i][2] * A[2][3] + inv[i][3] for i in range(3)]
    # sensor.yaml's 12 digits leave R orthonormal to 1e-12 only: Gram-Schmidt on its rows (+ - * / sqrt, as everything here)
    n0 = math.sqrt(R[0][0] * R[0][0] + R[0][1] * R[0][1] + R[0][2] * R[0][2])
    r0 = [R[0][0] / n0, R[0][1] / n0, R[0][2] / n0]
    d = r0[0] * R[1][0] + r0[1] * R[1][1] + r0[2] * R[1][2]
    r1 = [R[1][0] - d * r0[0], R[1][1] - d * r0[1], R[1][2] - d * r0[2]]
    n1 = math.sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2])
    r1 = [r1[0] / n1, r1[1] / n1, r1[2] / n1]
    R = [r0, r1, _cross(r0, r1)]
    c = [-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) for i in range(3)]
    baseline = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    ex = [c[0] / baseline, c[1] / baseline, c[2] / baseline]
    w = [R[2][0], R[2][1], 1.0 + R[2][2]]                       # z + R^T z
    ey = _cross(w, ex)
    n = math.sqrt(ey[0] * ey[0] + ey[1] * ey[1] + ey[2] * ey[2])
    ey = [ey[0] / n, ey[1] / n, ey[2] / n]
    ez = _cross(ex, ey)
    R1 = [ex, ey, ez]
    R2 = [[R1[i][0] * R[j][0] + R1[i][1] * R[j][1] + R1[i][2] * R[j][2] for j in range(3)] for i in range(3)]
    Kl, Kr = [float(v) for v in K_l], [float(v) for v in K_r]
    f = (Kl[1] + Kr[1]) / 2.0
    dflt = [f, f, (Kl[2] + Kr[2]) / 2.0, (Kl[3] + Kr[3]) / 2.0]
    nk = [0.0] * 4 if new_K is None else [float(v) for v in new_K]
    nk = tuple(dflt[k] if nk[k] == 0.0 else nk[k] for k in range(4))
    return dict(R1=np.array(R1), R2=np.array(R2), R=np.array(R), t=np.array(t), new_K=nk, baseline=baseline)


def _distort_terms(x, y, d):
    """rad, dx, dy of step 2 at normalised (x, y)."""
    k1, k2, p1, p2, k3 = d
    r2 = x * x + y * y
    rad = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return rad, dx, dy


_ATAN_C = tuple(np.float64(1.0) / np.float64(2 * k + 1) for k in range(13))             # 1 / (2k + 1), k = 0 .. 12
_TAN_S = tuple(np.float64((2 * k) * (2 * k + 1)) for k in range(9))                     # (2k)(2k + 1), k = 1 .. 8 used
_TAN_C = tuple(np.float64((2 * k - 1) * (2 * k)) for k in range(9))                     # (2k - 1)(2k)


def rect_atan(r):
    """atan(r) for r >= 0 from + - * / and sqrt: three half-angle steps t <- t / (1 + sqrt(1 + t t)) bring the argument
    under tan(pi / 16), then the Taylor series to t^25 in Horner form, times 8. Non-finite in, non-finite out; a finite r
    above 1.3e154, where t t overflows, gives 0 (on the device too): no ray of a finite calibration gets there."""
    t = np.asarray(r, np.float64)
    with np.errstate(all="ignore"):
        for _ in range(3):
            t = t / (1.0 + np.sqrt(1.0 + t * t))
        s = t * t
        p = _ATAN_C[12]
        for k in range(11, -1, -1):
            p = _ATAN_C[k] - s * p
        return 8.0 * (t * p)


def rect_tan(a):
    """tan(a) for 0 <= a < pi / 2 from + - * /: sin and cos of a / 8 by their Taylor series to h^17 and h^16 in Horner
    form, their quotient, three double-angle steps t <- 2 t / (1 - t t)."""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        h = a * 0.125
        s = h * h
        ps = pc = np.float64(1.0)
        for k in range(8, 0, -1):
            ps = 1.0 - s / _TAN_S[k] * ps
            pc = 1.0 - s / _TAN_C[k] * pc
        t = (h * ps) / pc
        for _ in range(3):
            t = (2.0 * t) / (1.0 - t * t)
        return t


def kb4_P(a, d):
    """P(a) = 1 + k1 a^2 + k2 a^4 + k3 a^6 + k4 a^8: the distorted angle is a P(a)."""
    k1, k2, k3, k4 = d[:4]
    q = a * a
    return (((k4 * q + k3) * q + k2) * q + k1) * q + 1.0


def kb4_D(a, d):
    """D(a) = d/da (a P(a)). D <= 0: the polynomial has folded back, the angle is beyond the lens's field."""
    k1, k2, k3, k4 = d[:4]
    q = a * a
    return (((9.0 * k4 * q + 7.0 * k3) * q + 5.0 * k2) * q + 3.0 * k1) * q + 1.0


def _kb4_scale(xn, yn, d):
    """Step 2k at normalised (xn, yn): (sc, D(a)) with xd = xn sc, yd = yn sc."""
    r = np.sqrt(xn * xn + yn * yn)
    a = rect_atan(r)
    sc = np.where(r == 0.0, 1.0, (a * kb4_P(a, d)) / r)
    return sc, kb4_D(a, d)


def _source_coords(cam, new_K, dst_w, dst_h):
    """Step 2 (2k) up to (su, sv, Z, model's own validity) for every destination pixel."""
    fx, fy, cx, cy = (np.float64(v) for v in cam["K"])
    nfx, nfy, ncx, ncy = (np.float64(v) for v in new_K)
    d = [np.float64(v) for v in cam["dist"]]
    R = [np.float64(v) for v in cam["R"]]
    u = np.arange(dst_w, dtype=np.float64)[None, :] + np.zeros((dst_h, 1))
    v = np.arange(dst_h, dtype=np.float64)[:, None] + np.zeros((1, dst_w))
    with np.errstate(all="ignore"):
        x, y = (u - ncx) / nfx, (v - ncy) / nfy
        X = R[0] * x + R[3] * y + R[6]
        Y = R[1] * x + R[4] * y + R[7]
        Z = R[2] * x + R[5] * y + R[8]
        xn, yn = X / Z, Y / Z
        if model_of(cam) == "kb4":
            sc, D = _kb4_scale(xn, yn, d)
            xd, yd = xn * sc, yn * sc
            ok = D > 0.0
        else:
            rad, dx, dy = _distort_terms(xn, yn, d)
            xd, yd = xn * rad + dx, yn * rad + dy
            ok = np.ones(Z.shape, bool)
        su, sv = fx * xd + cx, fy * yd + cy
    return su, sv, Z, ok


def source_coords(cam, new_K, dst_w, dst_h):
    """Step 2 (2k for a kb4 camera) up to (su, sv, Z) for every destination pixel, fp64 arrays of shape (dst_h, dst_w)."""
    return _source_coords(cam, new_K, dst_w, dst_h)[:3]


def fold_invalid(cam, new_K, dst_w, dst_h):
    """The destination pixels of a kb4 camera that step 2k's fold rule (D(a) <= 0) makes invalid, (dst_h, dst_w) bool."""
    return ~_source_coords(cam, new_K, dst_w, dst_h)[3]


def build_map(cam, new_K, src_w, src_h, dst_w, dst_h):
    """Step 2 (2k): the uint32 map (dst_h, dst_w): qx | qy << 16 in 1/32 px, or 0xFFFFFFFF."""
    su, sv, Z, ok_model = _source_coords(cam, new_K, dst_w, dst_h)
    with np.errstate(all="ignore"):
        qx, qy = np.floor(su * 32.0 + 0.5), np.floor(sv * 32.0 + 0.5)
        ok = ok_model & (Z > 0) & np.isfinite(su) & np.isfinite(sv)
        # ix >= 0 and ix + 1 <= Wsrc - 1 on the exact fp64 integers, before the conversion
        ok &= (qx >= 0) & (qy >= 0) & (qx < (src_w - 1) * 32.0) & (qy < (src_h - 1) * 32.0)
    q = np.where(ok, qx, 0).astype(np.int64) | (np.where(ok, qy, 0).astype(np.int64) << 16)
    return np.where(ok, q, INVALID).astype(np.uint32)


def remap(src, rmap, fill=0):
    """Step 3: one image (H, W) or a batch (n, H, W) through the map."""
    src = np.asarray(src, np.uint8)
    rmap = np.asarray(rmap, np.uint32)
    ok = rmap != INVALID
    m = np.where(ok, rmap, 0).astype(np.int64)
    qx, qy = m & 0xFFFF, m >> 16
    ix, iy, fx5, fy5 = qx >> 5, qy >> 5, qx & 31, qy & 31
    s = src.astype(np.int64)
    a, b = s[..., iy, ix], s[..., iy, ix + 1]
    c, d = s[..., iy + 1, ix], s[..., iy + 1, ix + 1]
    out = (a * (32 - fx5) * (32 - fy5) + b * fx5 * (32 - fy5) + c * (32 - fx5) * fy5 + d * fx5 * fy5 + 512) >> 10
    return np.where(ok, out, int(fill)).astype(np.uint8)


def distort(pts, cam):
    """Ideal pixel coordinates (n, 2) of a pinhole with the camera's K -> the raw (distorted) pixels. fp64."""
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = cam["K"]
    x, y = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    if model_of(cam) == "kb4":
        with np.errstate(all="ignore"):
            sc = _kb4_scale(x, y, [np.float64(v) for v in cam["dist"]])[0]
        return np.stack([fx * (x * sc) + cx, fy * (y * sc) + cy], axis=1)
    rad, dx, dy = _distort_terms(x, y, cam["dist"])
    return np.stack([fx * (x * rad + dx) + cx, fy * (y * rad + dy) + cy], axis=1)


def undistort_xy(xs, ys, cam, new_K):
    """Step 4 (4k) on fp64 raw pixel coordinates: (u', v', Z) as fp64, before the fp32 store and the validity rule. Under
    kb4 a point that step 4k's own rule rejects (the Newton run, the angle, the fold) has u' = v' = NaN."""
    fx, fy, cx, cy = (np.float64(v) for v in cam["K"])
    nfx, nfy, ncx, ncy = (np.float64(v) for v in new_K)
    d = [np.float64(v) for v in cam["dist"]]
    R = [np.float64(v) for v in cam["R"]]
    with np.errstate(all="ignore"):
        xd, yd = (np.asarray(xs, np.float64) - cx) / fx, (np.asarray(ys, np.float64) - cy) / fy
        if model_of(cam) == "kb4":
            td = np.sqrt(xd * xd + yd * yd)
            a = td
            for _ in range(FISHEYE_POINT_ITERATIONS):
                a = a - (a * kb4_P(a, d) - td) / kb4_D(a, d)
            ok = (np.isfinite(a) & (a >= 0.0) & (a < HALF_PI) & (kb4_D(a, d) > 0.0) &
                  (np.abs(a * kb4_P(a, d) - td) <= FISHEYE_RESIDUAL))
            sc = np.where(td == 0.0, 1.0, rect_tan(a) / td)
            x, y = np.where(ok, xd * sc, np.nan), np.where(ok, yd * sc, np.nan)
        else:
            x, y = xd, yd
            for _ in range(POINT_ITERATIONS):
                rad, dx, dy = _distort_terms(x, y, d)
                x, y = (xd - dx) / rad, (yd - dy) / rad
        X = R[0] * x + R[1] * y + R[2]
        Y = R[3] * x + R[4] * y + R[5]
        Z = R[6] * x + R[7] * y + R[8]
        return nfx * X / Z + ncx, nfy * Y / Z + ncy, Z


def undistort_points(kps, cam, new_K):
    """Step 4: KP_DTYPE records (or an (n, 2) array of raw pixels) moved into the undistorted / rectified frame. Records
    keep every other field; an fp32 array comes back as (n, 2) fp32 as the device writes it, an fp64 array as the fp64 values
    before that store."""
    k = np.asarray(kps)
    records = k.dtype == KP_DTYPE
    if records:
        out = k.reshape(-1).copy()
        xs, ys = out["x"], out["y"]
    else:
        p = np.asarray(kps).reshape(-1, 2)
        xs, ys = p[:, 0], p[:, 1]
    u, v, Z = undistort_xy(xs, ys, cam, new_K)
    if not records and p.dtype == np.float64:                   # fp64 in, fp64 out: the iteration itself, no fp32 store
        bad = ~((Z > 0) & np.isfinite(u) & np.isfinite(v))
        return np.stack([np.where(bad, -1.0, u), np.where(bad, -1.0, v)], axis=1)
    with np.errstate(all="ignore"):
        u32, v32 = u.astype(np.float32), v.astype(np.float32)
    bad = ~((Z > 0) & np.isfinite(u32) & np.isfinite(v32))
    u32[bad], v32[bad] = -1.0, -1.0
    if records:
        out["x"], out["y"] = u32, v32
        return out
    return np.stack([u32, v32], axis=1)


def scaled_calibration(W, H, full):
    """A calibration dict (K_l, K_r, D_l, D_r, T_BS_l, T_BS_r) with its intrinsics scaled from full["size"] to W x H."""
    sx, sy = W / full["size"][0], H / full["size"][1]
    sc = lambda K: (K[0] * sx, K[1] * sy, K[2] * sx, K[3] * sy)   # noqa: E731
    return dict(full, K_l=sc(full["K_l"]), K_r=sc(full["K_r"]), size=(W, H))


def rectified_cameras(calib, new_K=None):
    """(left camera, right camera, new_K, baseline) of a calibration dict: stereo_geometry's rotations attached. The dict
    may carry model ("radtan", the default, or "kb4"), which holds for both cameras."""
    g = stereo_geometry(calib["K_l"], calib["K_r"], calib["T_BS_l"], calib["T_BS_r"], new_K)
    m = calib.get("model", "radtan")
    return (camera(calib["K_l"], calib["D_l"], g["R1"], m), camera(calib["K_r"], calib["D_r"], g["R2"], m), g["new_K"],
            g["baseline"])


def _sample(img, u, v, outside):
    """Bilinear sample of a float image at fp64 (u, v); `outside` where a tap leaves the image or a coordinate is not finite."""
    H, W = img.shape
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, -1.0), np.where(ok, v, -1.0)
    x0, y0 = np.floor(u), np.floor(v)
    ok &= (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= W - 1) & (y0 + 1 <= H - 1)
    i, j = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
    fx, fy = u - x0, v - y0
    val = (img[j, i] * (1 - fx) + img[j, i + 1] * fx) * (1 - fy) + (img[j + 1, i] * (1 - fx) + img[j + 1, i + 1] * fx) * fy
    return np.where(ok, val, outside)


def raw_from_rectified(left, right, calib, new_K=None, outside=110.0):
    """A rectified pair (two gray images of one size) inverse-warped into the two distorted, rotated cameras of `calib`: every
    raw pixel is moved into the rectified frame by step 4 in fp64 and sampled there, bilinear; `outside` where the rectified
    image has no data. Returns (raw_left u8, raw_right u8)."""
    H, W = np.asarray(left).shape
    cam_l, cam_r, nk, _ = rectified_cameras(calib, new_K)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    raws = []
    for img, cam in ((left, cam_l), (right, cam_r)):
        u, v, Z = undistort_xy(xs, ys, cam, nk)
        val = _sample(np.asarray(img, np.float64), np.where(Z > 0, u, np.nan), np.where(Z > 0, v, np.nan), outside)
        raws.append(np.clip(np.rint(val), 0, 255).astype(np.uint8))
    return raws[0], raws[1]


def raw_stereo_pair(seed, W, H, calib, new_K=None, outside=110.0):
    """The raw views of stereo_ref.stereo_pair(seed, W, H) by raw_from_rectified. Returns (raw_left u8, raw_right u8, row
    disparities, rectified left, rectified right)."""
    from . import stereo_ref
    left, right, d = stereo_ref.stereo_pair(seed, W, H)
    raw_l, raw_r = raw_from_rectified(left, right, calib, new_K, outside)
    return raw_l, raw_r, d, left, right
