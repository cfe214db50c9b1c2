"""Undistortion and stereo rectification on the device (include/aria_orb_hip.h, "rectification"): the maps of one or two
cameras built at creation, image batches warped in HBM into the layout the batch extractor and the stereo stage read,
keypoints moved into the undistorted / rectified frame. The reference never applies its distortion coefficients;
aria_slam_amd.rectify_ref is the definition and the device equals it bit for bit. A handle's cameras are radtan or, with
model = "kb4", the fisheye model KB4 (OpenCV's "fisheye", Kalibr's "equidistant": k1..k4). Out of scope: Aria's FISHEYE624,
KB3, rays at or beyond 90 degrees from the axis, cylindrical and equirectangular destinations; parity with OpenCV's
fisheye:: functions is not pinned.

As with the other stages, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_batch_device call, or the rectifier must be created on the caller's stream."""
import ctypes as C

import numpy as np

from . import _lib, rectify_ref
from ._handle import StageHandle
from ._lib import KP_DTYPE, check
from .frontend import _ptr


def _numbers(line):
    """The numbers of a YAML flow sequence on one line: 'key: [a, b, c]' -> [a, b, c]."""
    lo, hi = line.find("["), line.rfind("]")
    if lo < 0:
        return []
    body = line[lo + 1:hi if hi > lo else len(line)]
    return [float(t) for t in body.replace(",", " ").split()]


def load_sensor_yaml(path, fisheye=False):
    """A camera's mav0/camN/sensor.yaml, read key by key and line by line as the reference's reader does (EuRoCReader
    loadCameraParams): `intrinsics: [fx, fy, cx, cy]`, `distortion_coefficients: [k1, k2, p1, p2(, k3)]`,
    `resolution: [w, h]`, and T_BS's 16-value `data: [...]` (which may run over several lines). Returns dict(K, dist
    (5 values), T_BS (4x4), resolution (w, h) or None, model). With fisheye = True the models `equidistant`, `fisheye` and
    `kb4` are accepted too: exactly four coefficients k1..k4 (dist = k1, k2, k3, k4, 0) and model = "kb4" in the dict."""
    out = dict(K=None, dist=None, T_BS=np.eye(4), resolution=None, model="radial-tangential")
    n_dist = 0
    with open(path) as f:
        lines = f.read().splitlines()
    in_tbs = False
    for n, line in enumerate(lines):
        if line.strip().startswith("T_BS"):
            in_tbs = True
        if "intrinsics:" in line:
            out["K"] = tuple(_numbers(line)[:4])
        elif "distortion_coefficients:" in line:
            n_dist = len(_numbers(line))
            d = _numbers(line)[:5]
            out["dist"] = tuple(d + [0.0] * (5 - len(d)))
        elif "distortion_model:" in line:
            out["model"] = line.split(":", 1)[1].strip()
        elif "resolution:" in line:
            out["resolution"] = tuple(int(v) for v in _numbers(line)[:2])
        elif "data:" in line and in_tbs:
            text = line
            k = n
            while "]" not in text and k + 1 < len(lines):
                k += 1
                text += " " + lines[k]
            v = _numbers(text)
            if len(v) != 16:
                raise ValueError("%s: T_BS data holds %d values, not 16" % (path, len(v)))
            out["T_BS"] = np.array(v, np.float64).reshape(4, 4)
            in_tbs = False
    if out["K"] is None or len(out["K"]) != 4:
        raise ValueError("%s: no intrinsics: [fx, fy, cx, cy]" % path)
    if out["dist"] is None:
        out["dist"] = (0.0,) * 5
    if fisheye and out["model"] in ("equidistant", "fisheye", "kb4"):
        if n_dist != 4:
            raise ValueError("%s: the %s model takes exactly 4 coefficients, the file has %d" % (path, out["model"], n_dist))
        out["model"] = "kb4"
        return out
    if out["model"] not in ("radial-tangential", "radtan", "plumb_bob"):
        raise ValueError("%s: distortion model %r is not radtan" % (path, out["model"]))
    return out


class HipRectifier(StageHandle):
    """Binding of aria_rect_t. cameras: one or two rectify_ref.camera dicts (K, dist, R, and model = "kb4" for a fisheye
    camera); new_K: intrinsics of the destination images (default: the first camera's K); src_size / dst_size: (width,
    height); model: "radtan" or "kb4" for camera dicts that do not say (default radtan). All cameras of a handle share one
    model: mixed models raise ValueError."""

    _prefix, _config = "rect", _lib.RectConfig

    def __init__(self, cameras=None, new_K=None, src_size=(752, 480), dst_size=None, fill=0, baseline=None, stream=None,
                 device=0, model=None):
        if isinstance(cameras, dict):
            cameras = [cameras]
        if model is not None and model not in rectify_ref.MODEL_NAMES:
            raise ValueError("model %r is neither 'radtan' nor 'kb4'" % (model,))
        # the keyword, then what the camera dicts say themselves: all of it must name one model
        models = {rectify_ref.MODEL_NAMES[model]} if model is not None else set()
        models |= {rectify_ref.model_of(cam) for cam in (cameras or []) if "model" in cam or model is None}
        if len(models) > 1:
            raise ValueError("the cameras of one rectifier share one distortion model, not %s" % " and ".join(sorted(models)))
        cfg = self._default_config(device, stream)
        cfg.model = rectify_ref.MODELS.index(models.pop() if models else "radtan")
        if cameras is not None:
            cfg.n_cameras = len(cameras)
            for k, cam in enumerate(cameras[:2]):
                c = cfg.cam[k]
                c.fx, c.fy, c.cx, c.cy = (float(v) for v in cam["K"])
                c.dist[:] = [float(v) for v in cam["dist"]]
                c.R[:] = [float(v) for v in cam["R"]]
        if new_K is None:
            new_K = (cfg.cam[0].fx, cfg.cam[0].fy, cfg.cam[0].cx, cfg.cam[0].cy)
        cfg.new_fx, cfg.new_fy, cfg.new_cx, cfg.new_cy = (float(v) for v in new_K)
        cfg.src_width, cfg.src_height = src_size
        cfg.dst_width, cfg.dst_height = src_size if dst_size is None else dst_size
        cfg.fill = fill
        self._baseline = baseline
        self._create(cfg)

    @classmethod
    def from_stereo_calibration(cls, K_l, D_l, T_BS_l, K_r, D_r, T_BS_r, src_size, dst_size=None, new_K=None, **kw):
        """Both cameras of a rig: aria_rect_stereo_geometry builds the rectifying rotations, the new intrinsics (entries of
        new_K that are zero or missing take the default) and the baseline."""
        L = _lib.load_library()
        cfg = _lib.RectConfig()
        if new_K is not None:
            cfg.new_fx, cfg.new_fy, cfg.new_cx, cfg.new_cy = (float(v) for v in new_K)
        a = lambda v, n: np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1)[:n])   # noqa: E731
        kl, kr, tl, tr = a(K_l, 4), a(K_r, 4), a(T_BS_l, 16), a(T_BS_r, 16)
        b = C.c_double(0.0)
        check(L.aria_rect_stereo_geometry(kl.ctypes.data, kr.ctypes.data, tl.ctypes.data, tr.ctypes.data, C.byref(cfg), C.byref(b)),
              "aria_rect_stereo_geometry")
        pad = lambda d: tuple(float(v) for v in d) + (0.0,) * (5 - len(d))   # noqa: E731
        cams = [dict(K=tuple(kl), dist=pad(D_l), R=tuple(cfg.cam[0].R)), dict(K=tuple(kr), dist=pad(D_r), R=tuple(cfg.cam[1].R))]
        if kw.get("model") is not None and rectify_ref.MODEL_NAMES.get(kw["model"]) == "kb4" and (len(D_l) != 4 or len(D_r) != 4):
            raise ValueError("kb4 takes exactly k1, k2, k3, k4")
        return cls(cams, (cfg.new_fx, cfg.new_fy, cfg.new_cx, cfg.new_cy), src_size, dst_size, baseline=b.value, **kw)

    @property
    def new_K(self):
        c = self.config
        return (c.new_fx, c.new_fy, c.new_cx, c.new_cy)

    @property
    def baseline(self):
        """Length of the stereo baseline in the unit of T_BS (None for a rectifier not made from a stereo calibration)."""
        return self._baseline

    @property
    def src_size(self):
        return (self.config.src_width, self.config.src_height)

    @property
    def dst_size(self):
        return (self.config.dst_width, self.config.dst_height)

    def camera(self, cam):
        c = self.config.cam[cam]
        out = dict(K=(c.fx, c.fy, c.cx, c.cy), dist=tuple(c.dist), R=tuple(c.R))
        if self.model == "kb4":
            out["model"] = "kb4"
        return out

    @property
    def model(self):
        """"radtan" or "kb4"."""
        return rectify_ref.MODELS[self.config.model]

    def map(self, cam=0):
        """The camera's map as a (dst_height, dst_width) uint32 array: qx | qy << 16 in 1/32 px, 0xFFFFFFFF = invalid."""
        w, h = self.dst_size
        out = np.zeros((h, w), np.uint32)
        n = self._L.aria_rect_get_map(self._h, cam, out.ctypes.data, out.size)
        if n < 0:
            check(n, "aria_rect_get_map")
        return out

    def remap(self, img, cam=0):
        """One gray image from a host array; blocks. Returns the (dst_height, dst_width) uint8 image."""
        im = np.asarray(img, np.uint8)
        w, h = self.src_size
        if im.shape != (h, w):
            raise ValueError("the image must be gray and %d x %d" % (w, h))
        if im.strides[1] != 1 or im.strides[0] < w:
            im = np.ascontiguousarray(im)
        dw, dh = self.dst_size
        out = np.empty((dh, dw), np.uint8)
        check(self._L.aria_rect_remap(self._h, cam, im.ctypes.data, im.strides[0], out.ctypes.data, dw), "aria_rect_remap")
        return out

    def remap_batch_device(self, d_src, n_frames, d_dst, cam=0, src_stride=None, src_pitch=None, dst_stride=None, dst_pitch=None):
        """aria_rect_remap_batch_device: device pointers (torch tensors or ints); pitches default to the widths and strides
        to pitch * height. Enqueued on the handle's stream; check() synchronises."""
        (sw, sh), (dw, dh) = self.src_size, self.dst_size
        src_pitch = sw if src_pitch is None else src_pitch
        dst_pitch = dw if dst_pitch is None else dst_pitch
        src_stride = src_pitch * sh if src_stride is None else src_stride
        dst_stride = dst_pitch * dh if dst_stride is None else dst_stride
        check(self._L.aria_rect_remap_batch_device(self._h, cam, _ptr(d_src), src_stride, src_pitch, n_frames, _ptr(d_dst),
                                                   dst_stride, dst_pitch), "aria_rect_remap_batch_device")

    def points(self, kps, cam=0):
        """One frame's keypoints (KP_DTYPE records, or a frame dict of OrbHipExtractor.extract) from host arrays; blocks.
        Returns the moved records."""
        k = kps["keypoints"] if isinstance(kps, dict) else kps
        k = np.ascontiguousarray(k)
        if k.dtype != KP_DTYPE:
            k = k.view(KP_DTYPE)
        k = k.reshape(-1)
        out = np.zeros(len(k), KP_DTYPE)
        if len(k):
            check(self._L.aria_rect_points(self._h, cam, k.ctypes.data, len(k), out.ctypes.data), "aria_rect_points")
        return out

    def points_batch_device(self, d_kp_in, d_n, kp_stride, n_frames, d_kp_out=None, cam=0):
        """aria_rect_points_batch_device: device pointers (torch tensors or ints); d_kp_out = None moves the keypoints in
        place. Enqueued on the handle's stream; check() synchronises and reports deferred errors."""
        check(self._L.aria_rect_points_batch_device(self._h, cam, _ptr(d_kp_in), _ptr(d_n), kp_stride, n_frames,
                                                    _ptr(d_kp_in if d_kp_out is None else d_kp_out)),
              "aria_rect_points_batch_device")


def algorithmic_bytes(dst_w, dst_h):
    return _lib.load_library().aria_rect_algorithmic_bytes(dst_w, dst_h)
