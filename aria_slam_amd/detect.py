"""The object-detector stage around the network (include/aria_orb_hip.h, "object detector"): the reference's IObjectDetector
port (include/interfaces/IObjectDetector.hpp:10-46) with TRTInference::preprocess and ::postprocess
(src/legacy/TRTInference.cpp:68-142) as kernels, batched over frames. aria_slam_amd.detect_ref restates both in NumPy and is
the definition; the device is bitwise equal to it.

The network is not part of this package. It is injected: `model` is any callable from a (B, 3, h, w) CUDA tensor (float32,
or float16 with half=True) to a (B, n_cand, 6) float32 CUDA tensor of rows [x1, y1, x2, y2, confidence, class_id] in
network-input coordinates -- a torch module on ROCm, or a stand-in. The tensor it receives is the buffer the preprocess
kernel wrote and the tensor it returns is read by the postprocess kernel where it lies: no copies. Without a model only the
device-only calls work; detect() raises, it never substitutes anything for a missing network.

Stream ordering -- which of the two possible answers was chosen. The model runs on torch's CURRENT stream; the kernels run on
the handle's stream (its own non-blocking one, or a borrowed one). Borrowing torch's stream is not a general answer: torch's
default stream is the legacy stream, whose handle is 0 and which therefore cannot be borrowed (aria_orb_config.stream).
So detect_batch_device (and the port-shaped calls on top of it) ALWAYS order the three steps with events:
    handle stream waits for torch's stream   (the images, wherever torch produced them)
    preprocess on the handle's stream  -> event -> torch's stream waits
    model on torch's stream            -> event -> handle's stream waits
    postprocess on the handle's stream -> event -> torch's stream waits
so the whole call behaves as if it had been enqueued on torch's current stream: no manual synchronisation before or after,
and torch operations that read the results are ordered behind it. Work queued on OTHER handles' streams (e.g.
flag_keypoints_device on an extractor's stream) is not ordered by this: pass that call the detector's stream, or sync().
preprocess_batch_device / postprocess_batch_device on their own only enqueue on the handle's stream, like every other
*_device call of the package."""
import ctypes as C

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import BOX_DTYPE, DETECTION_DTYPE, check
from .detect_ref import ALL_CLASSES, DYNAMIC_CLASSES
from .frontend import _ptr

__all__ = ["HipObjectDetector", "DETECTION_DTYPE", "BOX_DTYPE", "DYNAMIC_CLASSES", "ALL_CLASSES"]


def resize_table(src, dst):
    """(first tap, weight of the second tap in 1/2048) per destination index: aria_det_resize_table (host-only)."""
    buf = np.zeros(dst, np.uint32)
    n = _lib.load_library().aria_det_resize_table(src, dst, buf.ctypes.data, len(buf))
    if n < 0:
        raise _lib.AriaError(n, "aria_det_resize_table")
    return (buf[:n] & 0xFFFF).astype(np.int32), (buf[:n] >> 16).astype(np.int32)


class HipObjectDetector(StageHandle):
    """Binding of aria_det_t; the Python mirror of aria::adapters::hip::HipObjectDetector."""

    _prefix, _config = "det", _lib.DetConfig

    def __init__(self, model=None, input_size=(640, 640), stream=None, device=0, max_batch=1, half=False, dynamic_classes=None,
                 max_candidates=300):
        cfg = self._default_config(device, stream)
        cfg.input_w, cfg.input_h = int(input_size[0]), int(input_size[1])
        cfg.max_batch = max_batch
        cfg.max_candidates = max_candidates
        cfg.out_half = int(bool(half))
        self.model = model
        self.dynamic_classes = dynamic_classes
        self._create(cfg)
        self._input = None
        self._out = None
        self._pending = None
        self._raw = None

    def status(self):
        """(aria_det_check's status, detection rows needed, box rows needed), without raising."""
        nd, nb = C.c_int(), C.c_int()
        rc = self._L.aria_det_check(self._h, C.byref(nd), C.byref(nb))
        return rc, nd.value, nb.value

    def check(self):
        """Synchronise the handle's stream; raise when a frame's lists were truncated at det_cap / box_cap."""
        check(self.status()[0], "aria_det_check")

    def sync(self):
        """IObjectDetector::sync (IObjectDetector.hpp:45)."""
        self.check()

    # ---- device-only calls
    def _classes(self, dynamic_classes):
        dc = self.dynamic_classes if dynamic_classes is None else dynamic_classes
        if dc is None:
            return None, 0, None
        if isinstance(dc, str):
            assert dc == ALL_CLASSES
            return None, -1, None
        ids = np.ascontiguousarray(list(dc), np.int32)
        return ids.ctypes.data, len(ids), ids

    def input_tensor(self, n_frames=None):
        """The network-input buffer the preprocess kernel writes: a (max_batch, 3, h, w) torch tensor (or its first n_frames)."""
        import torch
        if self._input is None:
            c = self.config
            self._input = torch.empty((c.max_batch, 3, c.input_h, c.input_w), dtype=torch.float16 if c.out_half else torch.float32,
                                      device="cuda:%d" % c.device)
        return self._input if n_frames is None else self._input[:n_frames]

    def preprocess_batch_device(self, d_images, n_frames, width, height, d_input=None, channels=1, swap_rb=True, row_stride=None,
                                frame_stride=None):
        """aria_det_preprocess_batch_device. d_input None: the handle's input_tensor(); returns the tensor / pointer written."""
        row_stride = width * channels if row_stride is None else row_stride
        frame_stride = row_stride * height if frame_stride is None else frame_stride
        dst = self.input_tensor(n_frames) if d_input is None else d_input
        check(self._L.aria_det_preprocess_batch_device(self._h, _ptr(d_images), n_frames, width, height, row_stride, frame_stride,
                                                       channels, int(bool(swap_rb)), _ptr(dst)), "aria_det_preprocess_batch_device")
        return dst

    def postprocess_batch_device(self, d_raw, n_frames, n_candidates, src_width, src_height, d_dets, d_ndets, det_cap, d_boxes=None,
                                 d_nboxes=None, box_cap=0, conf=0.5, nms=0.45, dynamic_classes=None):
        """aria_det_postprocess_batch_device. Enqueued on the handle's stream; check() synchronises."""
        p, n, keep = self._classes(dynamic_classes)
        check(self._L.aria_det_postprocess_batch_device(self._h, _ptr(d_raw), n_frames, n_candidates, src_width, src_height, conf, nms,
                                                        p, n, _ptr(d_dets), _ptr(d_ndets), det_cap, _ptr(d_boxes), _ptr(d_nboxes),
                                                        box_cap), "aria_det_postprocess_batch_device")
        del keep

    def _run_model(self, x):
        import torch
        if self.model is None:
            raise RuntimeError("HipObjectDetector: no network was injected (model=None); there is no built-in one")
        raw = self.model(x)
        if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.float32 and raw.dim() == 3 and
                raw.shape[0] == x.shape[0] and raw.shape[2] == 6 and raw.shape[1] <= self.config.max_candidates):
            raise ValueError("the model must return a (B, n_cand <= %d, 6) float32 CUDA tensor" % self.config.max_candidates)
        return raw.contiguous()

    def _order(self, first, then):
        """`then` waits for what has been enqueued on `first` so far (torch streams); nothing when they are one stream."""
        import torch
        if first.cuda_stream == then.cuda_stream:
            return
        ev = torch.cuda.Event()
        ev.record(first)
        then.wait_event(ev)

    def _streams(self):
        import torch
        dev = "cuda:%d" % self.config.device
        return torch.cuda.current_stream(dev), torch.cuda.ExternalStream(self.stream, device=dev)

    def detect_batch_device(self, d_images, n_frames, width, height, d_dets, d_ndets, d_boxes=None, d_nboxes=None, det_cap=None,
                            box_cap=None, channels=1, swap_rb=True, row_stride=None, frame_stride=None, conf=0.5, nms=0.45,
                            dynamic_classes=None):
        """Preprocess, the injected model, postprocess -- ordered with events as the module docstring says. Frame f's rows go
        to d_dets + f * det_cap (default max_candidates) and d_ndets[f], the dynamic subset to d_boxes + f * box_cap and
        d_nboxes[f]. Returns the raw (n_frames, n_cand, 6) tensor the model produced (kept alive by the object until the next
        call)."""
        cap = self.config.max_candidates
        det_cap = cap if det_cap is None else det_cap
        box_cap = cap if box_cap is None else box_cap
        ts, hs = self._streams()
        self._order(ts, hs)
        x = self.preprocess_batch_device(d_images, n_frames, width, height, None, channels, swap_rb, row_stride, frame_stride)
        self._order(hs, ts)
        raw = self._run_model(x)
        self._order(ts, hs)
        self._raw = raw
        self.postprocess_batch_device(raw, n_frames, raw.shape[1], width, height, d_dets, d_ndets, det_cap, d_boxes, d_nboxes, box_cap,
                                      conf, nms, dynamic_classes)
        self._order(hs, ts)
        return raw

    # ---- IObjectDetector (include/interfaces/IObjectDetector.hpp:21-45): one host image in, records out
    def _out_buffers(self):
        import torch
        if self._out is None:
            c, dev = self.config, "cuda:%d" % self.config.device
            n = c.max_batch * c.max_candidates
            self._out = (torch.empty(n * DETECTION_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                         torch.empty(c.max_batch, dtype=torch.int32, device=dev),
                         torch.empty(n * BOX_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                         torch.empty(c.max_batch, dtype=torch.int32, device=dev))
        return self._out

    def detectAsync(self, image, swap_rb=True):
        """IObjectDetector::detectAsync (:31-35; TRTInference.cpp:171-192): upload, preprocess and the model, nothing waited
        for. image: (H, W) or (H, W, 3) uint8 (the port documents RGB; swap_rb as TRTInference::preprocess, :75)."""
        import torch
        img = np.ascontiguousarray(image, np.uint8)
        assert img.ndim in (2, 3) and (img.ndim == 2 or img.shape[2] == 3)
        H, W = img.shape[:2]
        ch = 1 if img.ndim == 2 else 3
        d_img = torch.from_numpy(img).to("cuda:%d" % self.config.device)
        ts, hs = self._streams()
        self._order(ts, hs)
        x = self.preprocess_batch_device(d_img, 1, W, H, None, ch, swap_rb)
        self._order(hs, ts)
        raw = self._run_model(x)
        self._pending = (d_img, raw, W, H)

    def getDetections(self, conf=0.5, nms=0.45, boxes=False):
        """IObjectDetector::getDetections (:38-42; TRTInference.cpp:195-199): postprocess of the pending frame with these
        thresholds; returns DETECTION_DTYPE records (and the dynamic-class BOX_DTYPE records with boxes=True)."""
        if self._pending is None:
            raise RuntimeError("getDetections without a pending detectAsync")
        _, raw, W, H = self._pending
        d_dets, d_nd, d_boxes, d_nb = self._out_buffers()
        cap = self.config.max_candidates
        ts, hs = self._streams()
        self._order(ts, hs)
        self.postprocess_batch_device(raw, 1, raw.shape[1], W, H, d_dets, d_nd, cap, d_boxes, d_nb, cap, conf, nms)
        self._order(hs, ts)
        self.check()
        nd, nb = int(d_nd[0].item()), int(d_nb[0].item())
        dets = d_dets[:nd * DETECTION_DTYPE.itemsize].cpu().numpy().view(DETECTION_DTYPE).copy()
        if not boxes:
            return dets
        return dets, d_boxes[:nb * BOX_DTYPE.itemsize].cpu().numpy().view(BOX_DTYPE).copy()

    def detect(self, image, conf=0.5, nms=0.45, swap_rb=True, boxes=False):
        """IObjectDetector::detect (:21-28; TRTInference.cpp:145-168)."""
        self.detectAsync(image, swap_rb)
        return self.getDetections(conf, nms, boxes)

    # ---- blocking host forms of the two stages (no model involved)
    def preprocess(self, image, swap_rb=True):
        """aria_det_preprocess: one host image -> (3, h, w) float32 / float16 array."""
        img = np.ascontiguousarray(image, np.uint8)
        H, W = img.shape[:2]
        ch = 1 if img.ndim == 2 else 3
        c = self.config
        out = np.empty((3, c.input_h, c.input_w), np.float16 if c.out_half else np.float32)
        check(self._L.aria_det_preprocess(self._h, img.ctypes.data, W, H, W * ch, ch, int(bool(swap_rb)), out.ctypes.data),
              "aria_det_preprocess")
        return out

    def postprocess(self, raw, src_width, src_height, conf=0.5, nms=0.45, dynamic_classes=None):
        """aria_det_postprocess: one frame's (n_cand, 6) host rows -> (DETECTION_DTYPE records, BOX_DTYPE records)."""
        raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 6)
        cap = max(len(raw), 1)
        dets, boxes = np.zeros(cap, DETECTION_DTYPE), np.zeros(cap, BOX_DTYPE)
        nd, nb = C.c_int(), C.c_int()
        p, n, keep = self._classes(dynamic_classes)
        check(self._L.aria_det_postprocess(self._h, raw.ctypes.data if len(raw) else None, len(raw), src_width, src_height, conf, nms,
                                           p, n, dets.ctypes.data, cap, C.byref(nd), boxes.ctypes.data, cap, C.byref(nb)),
              "aria_det_postprocess")
        del keep
        return dets[:nd.value].copy(), boxes[:nb.value].copy()
