"""Two-view triangulation and point map on the MI355X (aria_map_*, kernels in aria_slam_amd/csrc/map_triangulate.hip): ground
truth, agreement with the NumPy restatement, batch == single and determinism, edge cases, the filters, the device chain
extract -> match -> pose -> map, and the C++ adapter and driver. tests/test_gpu_map_scale.py holds the many-pair and
large-arena paths.

Tolerance of the float fields: measured, not chosen. The yardstick is aria_slam_amd/map_ref.py run in np.longdouble (its own
epsilon in the Jacobi convergence test, 60 sweeps). For each scene below (tests/map_cases.py), GAP is the largest difference
between the restatement's fp64 run and that extended run over the kept points, measured on the CPU: X relative, err
absolute (pixels), quality relative. Against the extended run the device is allowed
  X, quality   10 * GAP of the scene: one decade for the device's acos, sqrt and division and another order of summation
  err (fp32)   one fp32 spacing from float32(extended err): a value 1e-13 off can flip one rounding, no more (derived)
  kept set     identical. tests/test_map_host.py holds every tested quantity of the extended run at least 1e-9 (relative)
               from its threshold on these seeds; the smallest such distance is the column "margin"
  integers     equal.

GAP as measured (tools/map_gap.py prints this table):
    scene    X (rel)    err (abs)  quality (rel)  margin    kept
    ref0     1.02e-14   1.80e-13   6.27e-13       1.5e-04   1320 of 2000
    ref1     7.42e-15   2.65e-13   7.76e-13       2.4e-04   1311 of 2000
    ref2     5.03e-15   1.76e-13   7.59e-13       2.3e-04   1273 of 2000
    ref3     4.47e-15   2.09e-13   5.40e-13       4.2e-04   1264 of 2000
    edges    1.07e-15   1.30e-13   4.62e-13       4.5e-01   200 of 200
    scale0   6.94e-15   2.10e-13   9.07e-13       6.5e-03   4871 of 6100
    scale1   5.90e-15   1.92e-13   1.20e-12       4.0e-03   4601 of 5720
    scale2   2.72e-15   2.28e-13   8.35e-13       4.9e-03   4658 of 5824
    scale3   2.70e-15   2.46e-13   1.23e-12       3.8e-03   4491 of 5524
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_cases   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
REC = 72
# measured on the CPU with the committed restatement (tools/map_gap.py); (X relative, err absolute, quality relative)
GAP = {
    "ref0": (1.02e-14, 1.80e-13, 6.27e-13),
    "ref1": (7.42e-15, 2.65e-13, 7.76e-13),
    "ref2": (5.03e-15, 1.76e-13, 7.59e-13),
    "ref3": (4.47e-15, 2.09e-13, 5.40e-13),
    "edges": (1.07e-15, 1.30e-13, 4.62e-13),
    "scale0": (6.94e-15, 2.10e-13, 9.07e-13),
    "scale1": (5.90e-15, 1.92e-13, 1.20e-12),
    "scale2": (2.72e-15, 2.28e-13, 8.35e-13),
    "scale3": (2.70e-15, 2.46e-13, 1.23e-12),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_views = map_cases.views


def _rel(a, b):
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def hold(name, got, kept):
    """The float fields of the device's records `got` against the extended run of scene `name`; kept: the scene's matches the
    records belong to, in order. Prints what the device showed, then asserts the bounds of this module's docstring."""
    f64, ext = map_cases.ref_runs(name)
    gx, _, gq = GAP[name]
    X, err, q = ext["X"][kept], ext["err"][kept], ext["quality"][kept]
    d = got["X"].astype(map_cases.EXT) - X
    dx = float((np.sqrt((d * d).sum(1)) / np.sqrt((X * X).sum(1))).max())
    dq = float((np.abs(got["quality"].astype(map_cases.EXT) - q) / q).max())
    e32 = err.astype(np.float32)
    de = np.abs(got["err"].astype(np.float64) - e32.astype(np.float64))
    off = int((de > 0).sum())
    same = int(((got["X"] == f64["X"][kept]).all(1) & (got["quality"] == f64["quality"][kept])).sum())
    print("%s: X rel %.2e (allowed %.2e)  quality rel %.2e (allowed %.2e)  err: %d of %d one fp32 spacing off, %d further;  "
          "%d of %d records have the fp64 restatement's X and quality bit for bit"
          % (name, dx, 10 * gx, dq, 10 * gq, off, de.size, int((de > np.spacing(e32)).sum()), same, len(got)))
    assert dx <= 10 * gx and dq <= 10 * gq
    assert (de <= np.spacing(e32)).all()


def test_ground_truth(aria):
    from aria_slam_amd import map_ref as M
    mp = aria.HipMapper()
    try:
        for k in range(4):
            E1, E2 = _views(k)
            kq, kt, m, Xw, _ = M.synth_scene(10 + k, 600, E1, E2, noise_px=0.0, depth=(1.0, 6.0))
            mp.clear()
            assert mp.triangulate(kq, kt, m, E1, E2) == 600
            pts = mp.read()
            assert np.array_equal(pts["match"], np.arange(600)) and np.array_equal(pts["id"], np.arange(600))
            assert _rel(pts["X"], Xw).max() < 1e-6                      # fp32 pixels bound it, not the solver
            # 0.5 px noise
            kq, kt, m, Xw, _ = M.synth_scene(20 + k, 600, E1, E2, noise_px=0.5, depth=(1.0, 6.0))
            mp.clear()
            n = mp.triangulate(kq, kt, m, E1, E2)
            pts = mp.read()
            assert n > 400 and np.median(_rel(pts["X"], Xw[pts["match"]])) < 0.01
            # random-pixel outliers are rejected
            kq, kt, m, Xw, truth = M.synth_scene(30 + k, 600, E1, E2, outlier_frac=0.3, depth=(1.0, 6.0))
            mp.clear()
            mp.triangulate(kq, kt, m, E1, E2)
            pts = mp.read()
            kept = np.zeros(600, bool)
            kept[pts["match"]] = True
            assert kept[~truth].mean() <= 0.05
    finally:
        mp.close()


def test_dyadic_scene_is_exact(aria):
    """Projections exact in fp32 (tests/test_map_host.py): the fp64 DLT recovers X to 1e-9."""
    from aria_slam_amd import map_ref as M
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE
    K = (512.0, 512.0, 320.0, 240.0)
    rng = np.random.default_rng(0)
    n = 64
    X = np.stack([rng.integers(-64, 64, n) / 64, rng.integers(-48, 48, n) / 64, 2.0 ** rng.integers(1, 4, n)], 1)
    E1 = M.extrinsics(np.eye(3), [0, 0, 0])
    E2 = M.extrinsics(np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), [-1, 0.5, 0])
    kq, kt = np.zeros(n, KP_DTYPE), np.zeros(n, KP_DTYPE)
    for kk, E in ((kq, E1), (kt, E2)):
        c = X @ E[:, :3].T + E[:, 3]
        kk["x"], kk["y"] = K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]
    m = np.zeros(n, MATCH_DTYPE)
    m["query_idx"] = m["train_idx"] = np.arange(n)
    mp = aria.HipMapper(K=K)
    try:
        assert mp.triangulate(kq, kt, m, E1, E2) == n
        assert _rel(mp.read()["X"], X).max() < 1e-9
    finally:
        mp.close()


def test_against_map_ref(aria):
    from aria_slam_amd import map_ref as M
    mp = aria.HipMapper()
    try:
        for k in range(4):
            kq, kt, m, E1, E2 = map_cases.ref_scene(k)
            img = ((np.arange(480 * 752) * 7 + k) % 256).astype(np.uint8).reshape(480, 752)
            mp.clear()
            mp.triangulate(kq, kt, m, E1, E2, image=img, pair_id=k)
            got = mp.read()
            kept = np.flatnonzero(map_cases.ref_runs("ref%d" % k)[1]["keep"])
            assert len(kept) > 500
            assert np.array_equal(got["match"], kept)                   # the kept set: identical, no margin
            want = M.triangulate_pair(kq, kt, m, E1, E2, image=img, pair=k)
            assert np.array_equal(want["match"], kept)
            for f in ("pair", "idx1", "idx2", "gray"):
                assert np.array_equal(got[f], want[f]), f
            assert np.array_equal(got["id"], np.arange(len(kept)))
            hold("ref%d" % k, got, kept)
    finally:
        mp.close()


def _pack(torch, pairs, cap, dev):
    """Device blocks for pairs [(kq, kt, m, E1, E2)]: keypoints at p*cap (24 B), matches at p*cap (12 B), 24 doubles each."""
    B = len(pairs)
    kq = np.zeros((B, cap, 24), np.uint8)
    kt = np.zeros((B, cap, 24), np.uint8)
    mm = np.zeros((B, cap, 12), np.uint8)
    ext = np.zeros((B, 24), np.float64)
    nq, nt, nm = (np.zeros(B, np.int32) for _ in range(3))
    for p, (a, b, m, E1, E2) in enumerate(pairs):
        kq[p, :len(a)] = a.view(np.uint8).reshape(-1, 24)
        kt[p, :len(b)] = b.view(np.uint8).reshape(-1, 24)
        mm[p, :len(m)] = m.view(np.uint8).reshape(-1, 12)
        ext[p, :12], ext[p, 12:] = np.asarray(E1).reshape(-1)[:12], np.asarray(E2).reshape(-1)[:12]
        nq[p], nt[p], nm[p] = len(a), len(b), len(m)
    t = lambda x: torch.from_numpy(x).to(dev)
    return dict(kq=t(kq), nq=t(nq), kt=t(kt), nt=t(nt), mm=t(mm), nm=t(nm), ext=t(ext))


def _batch(mp, b, cap, lo, hi, base=0, added=None, pose=None, use_ext=True):
    mp.triangulate_batch_device(b["kq"].data_ptr() + lo * cap * 24, b["nq"].data_ptr() + lo * 4,
                                b["kt"].data_ptr() + lo * cap * 24, b["nt"].data_ptr() + lo * 4, cap,
                                b["mm"].data_ptr() + lo * cap * 12, b["nm"].data_ptr() + lo * 4, hi - lo, cap,
                                d_extrinsics=b["ext"].data_ptr() + lo * 192 if use_ext else None,
                                d_pose=None if pose is None else pose.data_ptr() + lo * 192,
                                d_added=None if added is None else added.data_ptr() + lo * 4, pair_base=base + lo)


def _varied_pairs(n_pairs):
    from aria_slam_amd import map_ref as M
    rng = np.random.default_rng(3)
    pairs = []
    for p in range(n_pairs):
        n = int(rng.choice([0, 5, 8, 12, 40, 150, 300, 600]))
        E1, E2 = _views(p % 4)
        kq, kt, m, _, _ = M.synth_scene(200 + p, max(n, 1), E1, E2, outlier_frac=0.2, depth=(1.0, 30.0))
        pairs.append((kq[:n], kt[:n], m[:n], E1, E2))
    return pairs


def test_batch_equals_single_split_and_repeat(aria, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    P_, cap, base = 64, 600, 100
    pairs = _varied_pairs(P_)
    b = _pack(torch, pairs, cap, dev)
    torch.cuda.synchronize()
    runs = []
    mp = aria.HipMapper(capacity=1 << 15)
    try:
        for split in ((0, 64), (0, 17, 40, 64), (0, 64)):
            mp.clear()
            added = torch.full((P_,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for lo, hi in zip(split[:-1], split[1:]):
                _batch(mp, b, cap, lo, hi, base, added)
            mp.check()
            runs.append((mp.read().tobytes(), added.cpu().numpy()))
        assert runs[0][0] == runs[2][0] and np.array_equal(runs[0][1], runs[2][1])                             # run to run
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])                             # split
        mp.clear()
        counts = []
        for p, (kq, kt, m, E1, E2) in enumerate(pairs):
            counts.append(mp.triangulate(kq, kt, m, E1, E2, pair_id=base + p))
        assert mp.read().tobytes() == runs[0][0]                                                                # single
        assert np.array_equal(np.array(counts), runs[0][1]) and sum(counts) > 3000
    finally:
        mp.close()


def test_edges(aria, torch_cuda):
    from aria_slam_amd import _lib
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    E1, E2 = _views(1)
    pairs = map_cases.edges_pairs()                                                 # pair 0: no matches
    cap = 200
    b = _pack(torch, pairs, cap, dev)
    # pose records: pair 1 invalid, pair 2 at the gate (n_pose_inliers = 10), pair 3 above it
    rec = np.zeros(4, _lib.POSE_RESULT_DTYPE)
    R2, t2 = map_cases.relative_pose(E1, E2)                                        # view 2 relative to view 1
    for p in range(4):
        rec[p]["R"], rec[p]["t"], rec[p]["valid"], rec[p]["n_pose_inliers"] = R2.reshape(-1), t2, 1, 100
    rec[1]["valid"] = 0
    rec[2]["n_pose_inliers"] = 10
    pose = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    mp = aria.HipMapper()
    try:
        added = torch.full((4,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        _batch(mp, b, cap, 0, 4, added=added, pose=pose, use_ext=False)
        mp.check()
        a = added.cpu().numpy()
        assert a[0] == 0 and a[1] == 0 and a[2] == 0 and a[3] > 150
        pts = mp.read()
        assert (pts["pair"] == 3).all() and len(pts) == a[3]
        # with pose records the world frame is view 1's: the points are view-1 camera coordinates
        kept = np.flatnonzero(map_cases.ref_runs("edges")[1]["keep"])
        assert np.array_equal(pts["match"], kept) and np.array_equal(pts["idx1"], kept) and np.array_equal(pts["idx2"], kept)
        hold("edges", pts, kept)
        # an out-of-range index in pair 2: reported once, pair skipped, the others unaffected
        mp.clear()
        bad = pairs[2][2].copy()
        bad["train_idx"][17] = 200
        pairs2 = list(pairs)
        pairs2[2] = (pairs[2][0], pairs[2][1], bad, E1, E2)
        b2 = _pack(torch, pairs2, cap, dev)
        torch.cuda.synchronize()
        _batch(mp, b2, cap, 0, 4, added=added)
        assert mp.status() == _lib.ARIA_OK - 1                          # ARIA_E_INVALID
        assert mp.status() == _lib.ARIA_OK                              # reported once
        got = mp.read()
        assert not (got["pair"] == 2).any()
        mp2 = aria.HipMapper()
        for p in (1, 3):
            mp2.triangulate(*pairs[p], pair_id=p)
        assert got.tobytes() == mp2.read().tobytes()
        mp2.close()
        with pytest.raises(aria.AriaError):
            mp.triangulate(*pairs2[2])                                  # the host form rejects it up front
        # capacity: whole pairs in order while they fit
        big = aria.HipMapper()
        _batch(big, b, cap, 0, 4, added=added)
        big.check()
        full = [int(v) for v in added.cpu().numpy()]
        big.close()
        small = aria.HipMapper(capacity=300)
        torch.cuda.synchronize()
        _batch(small, b, cap, 0, 4, added=added)
        assert small.status() == _lib.ARIA_E_OUTPUT_TOO_SMALL
        assert small.status() == _lib.ARIA_OK
        a = added.cpu().numpy()
        assert a[1] == full[1] and a[2] == 0 and a[3] == 0 and full[1] <= 300 < full[1] + full[2]
        assert small.size() == full[1] and small.points_needed() == sum(full)
        need = small.points_needed()
        small.clear()                                                   # clear() also resets points_needed
        assert small.points_needed() == 0
        small.reserve(need)
        _batch(small, b, cap, 0, 4, added=added)
        small.check()
        assert small.size() == sum(full) and list(added.cpu().numpy()) == full
        assert np.array_equal(small.read()["id"], np.arange(sum(full)))
        small.close()
    finally:
        mp.close()


def test_filters_match_map_ref(aria):
    from aria_slam_amd import map_ref as M
    from aria_slam_amd._lib import KP_DTYPE
    E1, E2 = _views(2)
    mp = aria.HipMapper(max_depth=50.0)
    ref = M.Map()
    try:
        for k in range(3):
            kq, kt, m, _, _ = M.synth_scene(90 + k, 400, E1, E2, depth=(1.0, 4.0))
            # plant far points: the same pixel rays at 40-48 units
            far, fkt, fm, _, _ = M.synth_scene(95 + k, 6, E1, E2, depth=(40.0, 48.0), noise_px=0.0)
            kq2 = np.concatenate([kq, far]).astype(KP_DTYPE)
            kt2 = np.concatenate([kt, fkt]).astype(KP_DTYPE)
            fm = fm.copy()
            fm["query_idx"] += 400
            fm["train_idx"] += 400
            mm = np.concatenate([m, fm])
            assert mp.triangulate(kq2, kt2, mm, E1, E2, pair_id=k) == ref.triangulate(kq2, kt2, mm, E1, E2, pair=k)
        before = mp.read()
        assert len(before) == len(ref.points) and np.array_equal(before["id"], ref.points["id"])
        want = M.filter_outliers(before)
        assert len(want) < len(before)
        mp.filter_outliers()
        mp.check()
        got = mp.read()
        assert got.tobytes() == want.tobytes()
        want = M.filter_distance(got, 3.0)
        mp.filter_distance(3.0)
        assert mp.read().tobytes() == want.tobytes() and 0 < len(want) < len(got)
        # below 10 points: no-op
        mp.clear()
        kq, kt, m, _, _ = M.synth_scene(99, 9, E1, E2, depth=(1.0, 4.0), noise_px=0.0)
        mp.triangulate(kq, kt, m, E1, E2)
        m9 = mp.read()
        mp.filter_outliers()
        assert mp.read().tobytes() == m9.tobytes()
        # ids keep counting after a filter
        mp.triangulate(kq, kt, m, E1, E2)
        assert list(mp.read()["id"]) == list(range(len(m9) * 2))
    finally:
        mp.close()


def test_exports_write_the_reference_format(aria, tmp_path):
    from aria_slam_amd import map_ref as M
    E1, E2 = _views(0)
    kq, kt, m, _, _ = M.synth_scene(5, 50, E1, E2, depth=(1.0, 5.0))
    mp = aria.HipMapper()
    try:
        n = mp.triangulate(kq, kt, m, E1, E2)
        mp.export_ply(str(tmp_path / "m.ply"))
        mp.export_pcd(str(tmp_path / "m.pcd"))
        ply = open(tmp_path / "m.ply").read().splitlines()
        assert ply[2] == "element vertex %d" % n and ply[9] == "end_header" and len(ply) == 10 + n
        assert ply[10].split()[3:] == ["127", "127", "127"]
        pcd = open(tmp_path / "m.pcd").read().splitlines()
        assert pcd[9] == "POINTS %d" % n and len(pcd) == 11 + n and pcd[11].split()[3] == str(127 * 65793)
    finally:
        mp.close()


def test_device_chain_extract_match_pose_map(aria, torch_cuda):
    """synth_sequence -> batch extract -> batch match -> batch pose -> batch map (pose records, pose masks, view-1 images),
    all on one stream, equals aria_map_triangulate on the fetched data."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    W, H, NF = 640, 480, 2000
    seq = aria.synth_sequence(41, 3, W, H)
    B = len(seq)
    images = torch.from_numpy(seq).to(dev)
    work = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    e = aria.OrbHipExtractor(max_features=NF, stream=work.cuda_stream, max_width=W, max_height=H, max_batch=B)
    mt = aria.HipMatcher(stream=work.cuda_stream)
    pe = aria.HipPoseEstimator(stream=work.cuda_stream)
    mp = aria.HipMapper(stream=work.cuda_stream, min_pose_inliers=0)
    try:
        cap = e.kp_capacity()
        with torch.cuda.stream(work):
            kps = torch.zeros((B, cap, 24), dtype=torch.uint8, device=dev)
            desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
            counts = torch.zeros((B,), dtype=torch.int32, device=dev)
            matches = torch.zeros((B, cap, 12), dtype=torch.uint8, device=dev)
            nm = torch.zeros((B,), dtype=torch.int32, device=dev)
            out = torch.zeros((B - 1) * 192, dtype=torch.uint8, device=dev)
            mask = torch.zeros((B - 1) * cap, dtype=torch.uint8, device=dev)
            added = torch.zeros((B - 1,), dtype=torch.int32, device=dev)
        work.synchronize()
        e.extract_batch_device(images, B, W, H, kps, desc, counts, cap)
        mt.match_batch_device(desc.data_ptr() + cap * 32, counts.data_ptr() + 4, desc, counts, B - 1, cap * 32, 0.75, matches,
                              nm, cap)
        pe.estimate_batch_device(kps.data_ptr() + cap * 24, counts.data_ptr() + 4, kps, counts, cap, matches, nm, B - 1, cap,
                                 out, mask, query_is_first=False, pair_base=0)
        # view 1 = train = frame p (its image), view 2 = query = frame p + 1
        mp.triangulate_batch_device(kps.data_ptr() + cap * 24, counts.data_ptr() + 4, kps, counts, cap, matches, nm, B - 1, cap,
                                    d_pose=out, d_mask=mask, d_img=images, img_stride=W * H, width=W, height=H, pitch=W,
                                    d_added=added, query_is_first=False, pair_base=0)
        e.check()
        mt.sync()
        pe.check()
        mp.check()
        got = mp.read()
        c = counts.cpu().numpy()
        k = kps.cpu().numpy()
        mh = matches.cpu().numpy()
        nmh = nm.cpu().numpy()
        mk = mask.cpu().numpy()
        rec = np.frombuffer(out.cpu().numpy().tobytes(), aria._lib.POSE_RESULT_DTYPE)
        from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE
        host = aria.HipMapper(min_pose_inliers=0)
        want_added = []
        for p in range(B - 1):
            kq = k[p + 1, :c[p + 1]].copy().view(KP_DTYPE).reshape(-1)
            kt = k[p, :c[p]].copy().view(KP_DTYPE).reshape(-1)
            m = mh[p, :nmh[p]].copy().view(MATCH_DTYPE).reshape(-1)
            if not rec[p]["valid"] or rec[p]["n_pose_inliers"] <= 0:
                want_added.append(0)
                continue
            E2 = np.concatenate([rec[p]["R"].reshape(3, 3), rec[p]["t"].reshape(3, 1)], 1)
            E1 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
            want_added.append(host.triangulate(kq, kt, m, E1, E2, image=seq[p], mask=mk[p * cap:p * cap + nmh[p]],
                                               query_is_first=False, pair_id=p))
        assert got.tobytes() == host.read().tobytes()
        assert list(added.cpu().numpy()) == want_added
        host.close()
    finally:
        mp.close()
        pe.close()
        mt.close()
        e.close()


def test_cpp_map_selftest(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "map_selftest.cpp")
    exe = os.path.join(ROOT, "build", "map_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe, os.path.join(ROOT, "build", "map_selftest.ply")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    kv = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    n = int(kv["triangulate"][0])
    assert n == 205 and float(kv["triangulate"][1]) < 1e-5         # every point kept; relative error against the scene
    assert kv["observations"] == ["1", "2", "2"]                   # frame ids of the two views, 2 observations
    assert kv["descriptor"] == ["1"]                               # view 1's descriptor row
    assert int(kv["size"][0]) == 2 * n and kv["filtered"] == [str(2 * n - 10)] * 2   # the 2 x 5 far points go
    assert int(kv["ply"][0]) == int(kv["filtered"][0])


def test_euroc_frontend_map(aria, tmp_path):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 8, w=640, h=480)
    exe = os.path.join(PKG, "euroc_frontend")
    t1, t2, ply = (str(tmp_path / n) for n in ("a.txt", "b.txt", "m.ply"))
    plain = subprocess.run([exe, str(tmp_path), "1000", "--pose", t1], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    run = subprocess.run([exe, str(tmp_path), "1000", "--pose", t2, "--map", ply], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert open(t1, "rb").read() == open(t2, "rb").read()
    line = [l for l in run.stdout.splitlines() if l.startswith("map ")]
    assert len(line) == 1
    n = int(line[0].split()[1])
    text = open(ply).read().splitlines()
    assert text[0] == "ply" and text[2] == "element vertex %d" % n and len(text) == 10 + n
    for l in text[10:]:
        v = l.split()
        assert len(v) == 6 and all(np.isfinite(float(x)) for x in v[:3]) and v[3] == v[4] == v[5]
    bad = subprocess.run([exe, str(tmp_path), "1000", "--map", ply], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--pose" in bad.stderr
