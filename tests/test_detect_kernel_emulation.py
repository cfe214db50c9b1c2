"""The kernel source of aria_slam_amd/csrc/detect_stage.hip, compiled for the HOST and held bitwise to the restatement
(aria_slam_amd/detect_ref.py) on the shapes and cases tests/test_gpu_detect.py runs on the device.

The text of the file between "namespace {" and the C-ABI -- both kernels, their device functions and the table builder --
is pasted between tests/cpp/det_kernel_emu_head.inc (a shim: one std::thread per lane, __syncthreads() as a std::barrier,
__shared__ as a static) and det_kernel_emu_tail.inc (the launch geometry) and compiled with the clang++ that hipcc drives.
What this checks without a GPU is the indexing, the tail and alignment paths of the stores, the rank sort and the
barrier structure of the greedy pass; what it cannot check is the device's arithmetic and the streams: that is
tests/test_gpu_detect.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detect_cases as DC
from aria_slam_amd import detect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu():
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "detect_stage.hip")).read()
    body = src[src.index("namespace {"):src.index("// ---- C-ABI")]
    assert "k_det_preprocess" in body and "k_det_postprocess" in body and "det_build_table" in body
    parts = [open(os.path.join(ROOT, "tests", "cpp", n)).read() for n in ("det_kernel_emu_head.inc", "det_kernel_emu_tail.inc")]
    out_dir = os.path.join(ROOT, "build", "det_emu")
    os.makedirs(out_dir, exist_ok=True)
    cpp, so = os.path.join(out_dir, "det_emu.cpp"), os.path.join(out_dir, "libdet_emu.so")
    with open(cpp, "w") as f:
        f.write(parts[0] + body + parts[1])
    assert os.path.exists(CLANG), "the clang++ of the ROCm installation (the one hipcc drives) is needed"
    subprocess.check_call([CLANG, "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-w", "-o", so, cpp])
    L = C.CDLL(so)
    p, i, f = C.c_void_p, C.c_int, C.c_float
    L.emu_pre.argtypes = [p, i, i, i, i, C.c_int64, i, i, i, i, i, p]
    L.emu_post.argtypes = [p, i, i, f, f, f, f, p, i, p, p, i, p, p, i, p]
    return L


def _pre(L, imgs, in_w, in_h, swap, half, row_pad, frame_pad):
    B, H, W = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else 3
    row = imgs.reshape(B, H, -1)
    rs = row.shape[2] + row_pad
    fs = H * rs + frame_pad
    buf = np.full((B, fs), 0xA5, np.uint8)
    buf[:, :H * rs].reshape(B, H, rs)[:, :, :row.shape[2]] = row
    nbytes = B * 3 * in_w * in_h * (2 if half else 4)
    raw = np.zeros(nbytes + 64, np.uint8)
    off = (-raw.ctypes.data) % 16                                 # a 16-byte aligned output, as a device allocation is
    out = raw[off:off + nbytes].view(np.float16 if half else np.float32).reshape(B, 3, in_h, in_w)
    out[:] = -1
    L.emu_pre(buf.ctypes.data, B, W, H, rs, fs, ch, int(swap), in_w, in_h, int(half), out.ctypes.data)
    return out


@pytest.mark.parametrize("shape", [(37, 23, 16, 12), (5, 7, 16, 16), (16, 16, 16, 16), (37, 23, 18, 10), (21, 9, 7, 5), (94, 60, 80, 80)])
def test_preprocess_kernel_source_is_bitwise_the_restatement(emu, shape):
    W, H, in_w, in_h = shape
    for ch in (1, 3):
        rng = np.random.default_rng(W * 1000 + H * 10 + ch)
        imgs = rng.integers(0, 256, (3, H, W) if ch == 1 else (3, H, W, 3), dtype=np.uint8)
        for half in (False, True):
            for swap in (False, True):
                want = R.preprocess_ref(imgs, in_w, in_h, ch, swap, half)
                got = _pre(emu, imgs, in_w, in_h, swap, half, 5, 13)
                assert got.tobytes() == want.tobytes(), (shape, ch, half, swap, int((got != want).sum()))


def _post(L, raw, src_w=640, src_h=640, conf=0.5, nms=0.45, dynamic_classes=None, det_cap=None, box_cap=None):
    raw = np.ascontiguousarray(raw, np.float32)
    B, nc = raw.shape[:2]
    det_cap = max(nc, 1) if det_cap is None else det_cap
    box_cap = max(nc, 1) if box_cap is None else box_cap
    dets, boxes = np.zeros((B, det_cap), R.DETECTION_DTYPE), np.zeros((B, box_cap), R.BOX_DTYPE)
    nd, nb, err = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(4, np.int32)
    if dynamic_classes is None:
        ids = np.array(R.DYNAMIC_CLASSES, np.int32)
        nid = len(ids)
    elif isinstance(dynamic_classes, str):
        ids, nid = np.zeros(1, np.int32), -1
    else:
        ids = np.array(dynamic_classes, np.int32)
        nid = len(ids)
    sx, sy = np.float32(src_w) / np.float32(640), np.float32(src_h) / np.float32(640)
    rr = raw if raw.size else np.zeros(6, np.float32)
    L.emu_post(rr.ctypes.data, B, nc, sx, sy, conf, nms, ids.ctypes.data, nid, dets.ctypes.data, nd.ctypes.data, det_cap,
               boxes.ctypes.data, nb.ctypes.data, box_cap, err.ctypes.data)
    return [(dets[k, :nd[k]].copy(), boxes[k, :nb[k]].copy()) for k in range(B)], err.tolist()


def _same(g, w):
    return g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes()


def test_postprocess_kernel_source_on_the_case_table(emu):
    for name in sorted(DC.POST_CASES):
        raw, kw, _, _ = DC.POST_CASES[name]
        kw = dict(kw)
        got, err = _post(emu, raw[None], kw.pop("src_w", 640), kw.pop("src_h", 640), **kw)
        assert _same(got[0], DC.run_case_ref(name)) and err[0] == 0, name


def test_postprocess_kernel_source_on_generated_frames(emu):
    frames = np.stack([DC.disjoint_frame(), DC.nested_frame(), DC.random_frame(), DC.random_frame(300, 8, 48)])
    want = R.postprocess_batch_ref(frames, 640, 640, 640, 640)
    got, _ = _post(emu, frames)
    assert all(_same(g, w) for g, w in zip(got, want))
    pairs = DC.iou_pairs_frame()
    assert _same(_post(emu, pairs[None])[0][0], R.postprocess_ref(pairs, 640, 640, 640, 640))
    for nc in (1, 63, 64, 65, 257, 1024):
        raw = DC.random_frame(nc, 100 + nc, 96)
        assert _same(_post(emu, raw[None], 752, 480)[0][0], R.postprocess_ref(raw, 752, 480, 640, 640)), nc
    # truncation: the truncated rows and the rows needed
    got, err = _post(emu, frames[:3], det_cap=100, box_cap=50)
    assert err[:3] == [1, max(len(w[0]) for w in want[:3]), max(len(w[1]) for w in want[:3])]
    assert all(g[0].tobytes() == w[0][:100].tobytes() and g[1].tobytes() == w[1][:50].tobytes() for g, w in zip(got, want))
