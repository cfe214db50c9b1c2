"""The object-detector stage on the device (include/aria_orb_hip.h, "object detector") against its NumPy restatement
(aria_slam_amd/detect_ref.py), which is the definition.

Everything is compared BITWISE. Both stages are integer arithmetic, single correctly rounded fp32 and fp64 operations and
copies: there is no tolerance to measure, and none is used anywhere in this file."""
import os
import subprocess

import numpy as np
import pytest

import detect_cases as DC
from aria_slam_amd import detect_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARIA_E_INVALID, ARIA_E_OUTPUT_TOO_SMALL = -1, -5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def post(aria, torch):
    d = aria.HipObjectDetector(input_size=(640, 640), max_batch=8, max_candidates=1024)
    yield d
    d.close()


# ---- preprocess
def _pad_frames(imgs, row_pad, frame_pad):
    """(B, H, W[, 3]) -> bytes laid out with a row stride of W * C + row_pad and a frame stride of H * row_stride + frame_pad,
    the gaps filled with a value no pixel computation may pick up unnoticed."""
    B, H = imgs.shape[:2]
    row = imgs.reshape(B, H, -1)
    rs = row.shape[2] + row_pad
    fs = H * rs + frame_pad
    buf = np.full((B, fs), 0xA5, np.uint8)
    v = buf[:, :H * rs].reshape(B, H, rs)
    v[:, :, :row.shape[2]] = row
    return buf, rs, fs


def _run_pre(aria, torch, imgs, in_w, in_h, swap, half, row_pad=0, frame_pad=0, max_batch=None):
    B, H, W = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else 3
    buf, rs, fs = _pad_frames(imgs, row_pad, frame_pad)
    det = aria.HipObjectDetector(input_size=(in_w, in_h), max_batch=max_batch or B, half=half)
    try:
        d = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        out = det.preprocess_batch_device(d, B, W, H, None, ch, swap, rs, fs)
        det.check()
        return out.cpu().numpy()
    finally:
        det.close()


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("shape", [(37, 23, 16, 12), (5, 7, 16, 16), (16, 16, 16, 16), (37, 23, 18, 10), (21, 9, 7, 5)],
                         ids=["down_37x23_16x12", "up_5x7_16x16", "identity_16", "tail_in_w_18", "in_w_7"])
def test_preprocess_small_shapes_bitwise(aria, torch, shape, ch, half):
    """B = 3 different frames, a row stride larger than the row and a frame stride larger than the frame, both swap_rb."""
    W, H, in_w, in_h = shape
    rng = np.random.default_rng(W * 1000 + H * 10 + ch)
    imgs = rng.integers(0, 256, (3, H, W) if ch == 1 else (3, H, W, 3), dtype=np.uint8)
    for swap in (False, True):
        want = R.preprocess_ref(imgs, in_w, in_h, ch, swap, half)
        got = _run_pre(aria, torch, imgs, in_w, in_h, swap, half, row_pad=5, frame_pad=13, max_batch=4)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), (shape, ch, half, swap, int((got != want).sum()))
    if shape == (16, 16, 16, 16) and not half:
        plane = imgs if ch == 1 else imgs[..., 0]
        assert np.array_equal(got[:, 2 if ch == 3 else 0], plane.astype(np.float32) * np.float32(1.0 / 255.0))


def test_preprocess_packed_frames_equal_padded_frames(aria, torch):
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (2, 23, 37), dtype=np.uint8)
    a = _run_pre(aria, torch, imgs, 20, 12, True, False)
    b = _run_pre(aria, torch, imgs, 20, 12, True, False, row_pad=27, frame_pad=101)
    assert a.tobytes() == b.tobytes() == R.preprocess_ref(imgs, 20, 12, 1).tobytes()


def test_preprocess_one_real_frame_752x480_to_640x640(aria, torch):
    a, _ = aria.synth_frame_pair(3, 752, 480)
    got = _run_pre(aria, torch, a[None], 640, 640, True, False)
    assert got.tobytes() == R.preprocess_ref(a[None], 640, 640, 1).tobytes()


def test_host_form_of_preprocess(aria):
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    det = aria.HipObjectDetector(input_size=(18, 10))
    try:
        assert det.preprocess(img, swap_rb=True).tobytes() == R.preprocess_ref(img[None], 18, 10, 3, True)[0].tobytes()
        assert det.preprocess(img[..., 1], swap_rb=False).tobytes() == R.preprocess_ref(img[None, ..., 1], 18, 10, 1)[0].tobytes()
    finally:
        det.close()


# ---- postprocess
def _run_post(det, torch, raw, src_w=640, src_h=640, conf=0.5, nms=0.45, dynamic_classes=None, det_cap=None, box_cap=None):
    """raw (B, n, 6) -> ([(detections, boxes)] per frame, aria_det_check's (status, det rows needed, box rows needed))."""
    raw = np.ascontiguousarray(raw, np.float32)
    B, n = raw.shape[:2]
    det_cap = max(n, 1) if det_cap is None else det_cap
    box_cap = max(n, 1) if box_cap is None else box_cap
    d_raw = torch.from_numpy(raw).cuda() if raw.size else torch.zeros(6, device="cuda")
    d_dets = torch.full((B * det_cap * 24 + 24,), 0xEE, dtype=torch.uint8, device="cuda")
    d_boxes = torch.full((B * box_cap * 16 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    d_nd = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    d_nb = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.postprocess_batch_device(d_raw, B, n, src_w, src_h, d_dets, d_nd, det_cap, d_boxes, d_nb, box_cap, conf, nms, dynamic_classes)
    status = det.status()
    nd, nb = d_nd.cpu().numpy(), d_nb.cpu().numpy()
    hd, hb = d_dets.cpu().numpy(), d_boxes.cpu().numpy()
    assert (hd[B * det_cap * 24:] == 0xEE).all() and (hb[B * box_cap * 16:] == 0xEE).all()      # nothing past the lists
    hd = hd[:B * det_cap * 24].view(R.DETECTION_DTYPE).reshape(B, det_cap)
    hb = hb[:B * box_cap * 16].view(R.BOX_DTYPE).reshape(B, box_cap)
    return [(hd[f, :nd[f]].copy(), hb[f, :nb[f]].copy()) for f in range(B)], status


def _same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("name", sorted(DC.POST_CASES))
def test_postprocess_case_table_through_the_device(post, torch, name):
    raw, kw, _, _ = DC.POST_CASES[name]
    kw = dict(kw)
    want = DC.run_case_ref(name)
    got, status = _run_post(post, torch, raw[None], kw.pop("src_w", 640), kw.pop("src_h", 640), **kw)
    assert status[0] == 0 and _same(got[0], want), (name, got[0], want)
    # the blocking host form gives the same
    kw = dict(DC.POST_CASES[name][1])
    assert _same(post.postprocess(raw, kw.pop("src_w", 640), kw.pop("src_h", 640), **kw), want), name


def test_postprocess_generated_frames(post, torch):
    frames = {"disjoint": DC.disjoint_frame(), "nested": DC.nested_frame(), "random": DC.random_frame(),
              "random2": DC.random_frame(300, 8, 48)}
    raw = np.stack(list(frames.values()))
    want = R.postprocess_batch_ref(raw, 640, 640, 640, 640)
    got, status = _run_post(post, torch, raw)
    assert status[0] == 0
    for k, (name, g, w) in enumerate(zip(frames, got, want)):
        assert _same(g, w), name
    assert len(want[0][0]) == 300 and len(want[1][0]) == 1 and 1 < len(want[2][0]) < 300
    # disjoint: the order is the pure (score descending, index ascending) sort
    order = np.lexsort((np.arange(300), -frames["disjoint"][:, 4].astype(np.float64)))
    assert np.array_equal(got[0][0]["x1"], frames["disjoint"][order, 0])


def test_iou_one_pixel_either_side_of_the_threshold(post, torch):
    raw = DC.iou_pairs_frame()
    got, _ = _run_post(post, torch, raw[None])
    want = R.postprocess_ref(raw, 640, 640, 640, 640)
    assert _same(got[0], want)
    assert [int(np.nonzero(raw[:, 4] == c)[0][0]) for c in got[0][0]["confidence"]] == DC.IOU_PAIRS_KEPT


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 1024])
def test_postprocess_candidate_counts(post, torch, n):
    raw = DC.random_frame(n, 100 + n, 96)
    got, status = _run_post(post, torch, raw[None])
    assert status[0] == 0 and _same(got[0], R.postprocess_ref(raw, 640, 640, 640, 640)), n


def test_batch_of_five_with_an_empty_frame_and_position_independence(post, torch):
    full = [DC.random_frame(300, s, 64) for s in (21, 22, 23, 24)]
    empty = full[0].copy()
    empty[:, 4] = 0.0
    raw = np.stack([full[0], full[1], empty, full[2], full[3]])
    want = R.postprocess_batch_ref(raw, 752, 480, 640, 640)
    got, status = _run_post(post, torch, raw, 752, 480)
    assert status[0] == 0 and all(_same(g, w) for g, w in zip(got, want))
    assert len(got[2][0]) == 0 and len(got[2][1]) == 0 and len(got[1][0]) > 0 and len(got[3][0]) > 0
    # one frame alone, first and last in a batch: identical rows
    alone, _ = _run_post(post, torch, full[1][None], 752, 480)
    first, _ = _run_post(post, torch, np.stack([full[1], full[2], full[3]]), 752, 480)
    last, _ = _run_post(post, torch, np.stack([full[3], empty, full[1]]), 752, 480)
    assert _same(alone[0], want[1]) and _same(first[0], want[1]) and _same(last[2], want[1])


def test_truncation_is_reported_with_the_rows_needed(post, torch):
    raw = np.stack([DC.disjoint_frame(), DC.nested_frame(), DC.random_frame()])
    want = R.postprocess_batch_ref(raw, 640, 640, 640, 640)
    need_d, need_b = max(len(w[0]) for w in want), max(len(w[1]) for w in want)
    got, status = _run_post(post, torch, raw, det_cap=100, box_cap=50)
    assert status == (ARIA_E_OUTPUT_TOO_SMALL, need_d, need_b)
    for g, w in zip(got, want):
        assert g[0].tobytes() == w[0][:100].tobytes() and g[1].tobytes() == w[1][:50].tobytes()
    assert post.status() == (0, 0, 0)                             # reported once
    # only the boxes too small
    got, status = _run_post(post, torch, raw, det_cap=300, box_cap=50)
    assert status == (ARIA_E_OUTPUT_TOO_SMALL, 0, need_b) and all(g[0].tobytes() == w[0].tobytes() for g, w in zip(got, want))
    # d_boxes may be NULL
    d_raw = torch.from_numpy(raw).cuda()
    d_dets = torch.zeros(3 * 300 * 24, dtype=torch.uint8, device="cuda")
    d_nd = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    post.postprocess_batch_device(d_raw, 3, 300, 640, 640, d_dets, d_nd, 300)
    assert post.status() == (0, 0, 0) and d_nd.cpu().tolist() == [len(w[0]) for w in want]


def test_argument_errors_come_back_before_any_launch(aria, post, torch):
    L = aria.load_library()
    h = post._h
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    pre = lambda n=1, w=16, h_=16, rs=16, fs=256, ch=1: L.aria_det_preprocess_batch_device(h, p, n, w, h_, rs, fs, ch, 0, p)
    assert pre(ch=2) == ARIA_E_INVALID and pre(ch=4) == ARIA_E_INVALID
    assert pre(n=9) == ARIA_E_INVALID                                 # max_batch is 8
    assert pre(w=0) == ARIA_E_INVALID and pre(h_=-1) == ARIA_E_INVALID
    assert pre(rs=15) == ARIA_E_INVALID and pre(n=2, fs=255) == ARIA_E_INVALID
    assert pre(ch=3, rs=47) == ARIA_E_INVALID
    pst = lambda n=1, nc=300, w=16, h_=16: L.aria_det_postprocess_batch_device(h, p, n, nc, w, h_, 0.5, 0.45, None, 0, p, p, 4, None, None, 0)
    assert pst(nc=1025) == ARIA_E_INVALID and pst(n=9) == ARIA_E_INVALID and pst(w=0) == ARIA_E_INVALID and pst(nc=-1) == ARIA_E_INVALID
    ids = np.arange(40, dtype=np.int32)
    assert L.aria_det_postprocess_batch_device(h, p, 1, 300, 16, 16, 0.5, 0.45, ids.ctypes.data, 33, p, p, 4, None, None, 0) == ARIA_E_INVALID
    assert post.status() == (0, 0, 0)
    small = aria.HipObjectDetector(max_candidates=300)
    try:
        assert L.aria_det_postprocess_batch_device(small._h, p, 1, 301, 16, 16, 0.5, 0.45, None, 0, p, p, 4, None, None, 0) == ARIA_E_INVALID
    finally:
        small.close()


# ---- end to end on the device
W, H, NC = 640, 480, 300


class StandInNetwork:
    """A stand-in for the network: 300 candidate rows per frame derived from the input tensor, written on torch's CURRENT
    stream after some unrelated work (so a missing wait in front of the postprocess kernel would read a half-written head,
    and a missing wait in front of this callable would read a half-written input)."""

    def __init__(self, torch):
        self.torch = torch
        g = torch.Generator().manual_seed(5)
        self.ys = torch.randint(0, 640, (NC,), generator=g).cuda()
        self.xs = torch.randint(0, 640, (NC,), generator=g).cuda()
        self.burn = torch.rand((1024, 1024), generator=g).cuda() * 1e-3
        self.calls = 0

    def __call__(self, x):
        torch = self.torch
        self.calls += 1
        z = self.burn
        for _ in range(6):
            z = z @ self.burn
        v = x[:, 1].float()[:, self.ys, self.xs]                    # (B, 300) in [0, 1]
        u = x[:, 0].float()[:, self.xs, self.ys]
        cx, cy = self.xs.float()[None], self.ys.float()[None]
        hw, hh = 8 + 90 * u, 8 + 70 * v
        conf = torch.floor((0.2 + 0.8 * v) * 32) / 32                 # ties
        cls = torch.floor(u * 20)
        return torch.stack([cx - hw, cy - hh, cx + hw, cy + hh, conf, cls + 0 * z[0, 0]], dim=2).contiguous()


@pytest.mark.parametrize("stream_kind", ["own", "borrowed"])
def test_detect_batch_device_end_to_end(aria, torch, stream_kind):
    a, b = aria.synth_frame_pair(1, W, H)
    frames = np.stack([a, b, a[::-1].copy()])
    B = len(frames)
    net = StandInNetwork(torch)
    side = torch.cuda.Stream()
    det = aria.HipObjectDetector(model=net, input_size=(640, 640), max_batch=B, stream=side.cuda_stream if stream_kind == "borrowed" else None)
    ext = aria.OrbHipExtractor(max_features=500, max_width=W, max_height=H, max_batch=B)
    try:
        assert (det.stream == side.cuda_stream) == (stream_kind == "borrowed")
        cap = ext.kp_capacity()
        d_img = torch.from_numpy(frames).cuda()
        d_dets = torch.zeros(B * NC * 24, dtype=torch.uint8, device="cuda")
        d_boxes = torch.zeros(B * NC * 16, dtype=torch.uint8, device="cuda")
        d_nd = torch.zeros(B, dtype=torch.int32, device="cuda")
        d_nb = torch.zeros(B, dtype=torch.int32, device="cuda")
        # no manual synchronisation between the upload, the three steps and the reads below: detect_batch_device orders them
        raw = det.detect_batch_device(d_img, B, W, H, d_dets, d_nd, d_boxes, d_nb)
        h_raw = raw.cpu().numpy()
        nd, nb = d_nd.cpu().numpy(), d_nb.cpu().numpy()
        h_dets = d_dets.cpu().numpy().view(R.DETECTION_DTYPE).reshape(B, NC)
        h_boxes = d_boxes.cpu().numpy().view(R.BOX_DTYPE).reshape(B, NC)
        assert det.status() == (0, 0, 0) and net.calls == 1 and h_raw.shape == (B, NC, 6)
        # the network saw the preprocessed frames: the same callable on the restatement's tensor gives the same head
        want_in = R.preprocess_ref(frames, 640, 640, 1)
        assert det.input_tensor(B).cpu().numpy().tobytes() == want_in.tobytes()
        assert net(torch.from_numpy(want_in).cuda()).cpu().numpy().tobytes() == h_raw.tobytes()
        want = R.postprocess_batch_ref(h_raw, W, H, 640, 640)
        for f in range(B):
            assert h_dets[f, :nd[f]].tobytes() == want[f][0].tobytes(), f
            assert h_boxes[f, :nb[f]].tobytes() == want[f][1].tobytes(), f
        assert min(nb) > 0 and max(nd) < NC
        # the lists left in HBM flag the keypoints exactly as the restatement's boxes uploaded from the host
        kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device="cuda")
        desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ext.extract_batch_device(d_img, B, W, H, kps, desc, cnt, cap)
        ext.check()
        up_boxes = np.zeros((B, NC), R.BOX_DTYPE)
        for f in range(B):
            up_boxes[f, :len(want[f][1])] = want[f][1]
        d_up = torch.from_numpy(up_boxes.view(np.uint8).reshape(-1)).cuda()
        d_upn = torch.from_numpy(np.array([len(w[1]) for w in want], np.int32)).cuda()
        fl_dev = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
        fl_host = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        aria.flag_keypoints_device(ext.stream, kps, cnt, B, cap, d_boxes, d_nb, NC, 0, fl_dev)
        aria.flag_keypoints_device(ext.stream, kps, cnt, B, cap, d_up, d_upn, NC, 0, fl_host)
        ext.check()
        assert torch.equal(fl_dev, fl_host) and int(fl_dev.sum()) > 0
        # the port-shaped calls give the batch call's records
        for f in range(B):
            one = det.detect(frames[f])
            assert one.tobytes() == want[f][0].tobytes(), f
        det.detectAsync(frames[1])
        det.sync()
        dd, bb = det.getDetections(boxes=True)
        assert dd.tobytes() == want[1][0].tobytes() and bb.tobytes() == want[1][1].tobytes()
        looser = det.detect(frames[1], conf=0.3, nms=0.6)
        assert looser.tobytes() == R.postprocess_ref(h_raw[1], W, H, 640, 640, 0.3, 0.6)[0].tobytes() and len(looser) > len(dd)
    finally:
        det.close()
        ext.close()


def test_detect_without_a_model_is_an_error(aria, torch):
    det = aria.HipObjectDetector()
    try:
        with pytest.raises(RuntimeError, match="no network"):
            det.detect(np.zeros((48, 64), np.uint8))
    finally:
        det.close()


# ---- C++ adapter
def test_cpp_adapter_and_frontend_injection(aria, torch, tmp_path):
    exe = DC.build_selftest()
    # a fixed head: two big dynamic boxes over textured parts of the frame, overlapping and non-dynamic extras, ties
    table = np.array([[100, 120, 420, 520, 0.9, 0], [110, 130, 430, 530, 0.85, 0], [300, 40, 620, 300, 0.8, 2],
                      [10, 10, 60, 60, 0.7, 9], [10, 10, 60, 60, 0.7, 16], [500, 500, 630, 630, 0.5, 0],
                      [0, 300, 200, 639, 0.65, 15.7], [5, 5, 7, 7, 0.2, 0]], np.float32)
    rawfile = tmp_path / "head.txt"
    rawfile.write_text("\n".join(" ".join("%.9g" % v for v in row) for row in table) + "\n")
    out = subprocess.run([exe, "run", str(rawfile), "1", str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    kv = {l[0]: l[1:] for l in lines if l[0] not in ("det", "fe")}
    a, b = aria.synth_frame_pair(1, W, H)
    d_table = torch.from_numpy(table).cuda()
    det = aria.HipObjectDetector(model=lambda x: d_table[None].expand(x.shape[0], -1, -1).contiguous(), max_candidates=len(table))
    try:
        py, py_boxes = det.detect(a, boxes=True)
    finally:
        det.close()
    want = R.postprocess_ref(table, W, H, 640, 640)
    assert py.tobytes() == want[0].tobytes() and py_boxes.tobytes() == want[1].tobytes()
    cpp = [l[1:] for l in lines if l[0] == "det"]
    assert len(cpp) == len(py)
    for row, d in zip(cpp, py):
        assert [float(v) for v in row[1:5]] == [d["x1"], d["y1"], d["x2"], d["y2"]]
        assert int(row[5], 16) == int(np.float32(d["confidence"]).view(np.uint32)) and int(row[6]) == d["class_id"]
    assert kv["nboxes"] == [str(len(py_boxes))] and kv["rgb_same"] == ["1"] and kv["async_same"] == ["1"] and kv["check"] == ["0"]
    # FrontEnd with the detector injected == setDetections() by hand with that detector's output, and the filter did something
    fe = [l[1:] for l in lines if l[0] == "fe"]
    inj, hand = [r[1:] for r in fe if r[0] == "injected"], [r[1:] for r in fe if r[0] == "byhand"]
    assert len(inj) == 3 and inj == hand and kv["fe_same"] == ["1"]
    assert inj[0][1:3] == ["0", "0"] and int(inj[1][1]) > 0 and int(inj[1][2]) > 0
