"""Ray casting of the volume (include/aria_orb_hip.h, "ray casting of the volume"): the parts that need no GPU -- exports, the
layouts, defaults and validation, and the NumPy restatement (aria_slam_amd/ray_ref.py, which is the definition) on known
answers and against the analytic scene of tests/tsdf_cases.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_cases as RC   # noqa: E402
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import ray_ref as R   # noqa: E402

RAY_SYMBOLS = ["aria_ray_default_config", "aria_ray_create", "aria_ray_destroy", "aria_ray_stream", "aria_ray_check",
               "aria_ray_update_from_volume_device", "aria_ray_cast_batch_device", "aria_ray_cast", "aria_ray_algorithmic_bytes"]
f32 = np.float32


def test_ray_symbols_exported_and_listed(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    header = open(os.path.join(ROOT, "include", "aria_orb_hip.h")).read()
    for name in RAY_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s not declared in the header" % name
        assert hasattr(L, name), "libaria_orb_hip.so does not export %s" % name
        assert name in _lib.EXPORTS, "%s missing from _lib.EXPORTS" % name
    assert aria.abi_version() == 4
    assert "HipVolumeRenderer" in aria.__all__
    assert "aria_ray_config;              /* 96 bytes" in header and "aria_ray_view;                /* 16 bytes" in header


def test_ray_layouts_and_defaults(aria):
    from aria_slam_amd import _lib
    L = aria.load_library()
    assert C.sizeof(_lib.RayConfig) == 96
    assert _lib.RAY_VIEW_DTYPE.itemsize == 16 and _lib.RAY_VIEW_DTYPE == R.VIEW_DTYPE
    cfg = _lib.RayConfig()
    L.aria_ray_default_config(C.byref(cfg))
    assert cfg.struct_size == 96 and not cfg.stream
    assert (cfg.nx, cfg.ny, cfg.nz, cfg.min_weight, cfg.skip) == (256, 256, 128, 2, 1)
    assert (cfg.voxel, cfg.near, cfg.far, cfg.step) == (f32(0.05), f32(0.3), f32(10.0), f32(0.05))
    assert (cfg.fx, cfg.fy, cfg.cx, cfg.cy) == (458.654, 457.296, 367.215, 248.375)
    d = R.config()
    assert d.dims == (256, 256, 128) and (d.voxel, d.near, d.far, d.step) == (cfg.voxel, cfg.near, cfg.far, cfg.step)
    assert tuple(d.origin) == tuple(f32(v) for v in cfg.origin) and (d.min_weight, d.skip) == (2, 1) and d.K == R.EUROC_K
    assert R.n_steps(d) == 195                                       # floorf(9.7f / 0.05f) + 1
    # the volume's defaults are this stage's defaults
    t = _lib.TsdfConfig()
    L.aria_tsdf_default_config(C.byref(t))
    assert (t.nx, t.ny, t.nz, t.min_weight, t.voxel, tuple(t.origin)) == (cfg.nx, cfg.ny, cfg.nz, cfg.min_weight, cfg.voxel, tuple(cfg.origin))
    assert (t.fx, t.fy, t.cx, t.cy) == (cfg.fx, cfg.fy, cfg.cx, cfg.cy)
    for planes, per in ((15, 18), (1, 4), (2, 12), (4, 1), (8, 1), (0, 0), (9, 5)):
        want = (per * 752 * 480 + 16) * 32
        assert L.aria_ray_algorithmic_bytes(752, 480, 32, planes) == want == R.algorithmic_bytes(752, 480, 32, planes)
    assert L.aria_ray_algorithmic_bytes(0, 480, 1, 15) == -1 and L.aria_ray_algorithmic_bytes(752, 16385, 1, 15) == -1
    assert L.aria_ray_algorithmic_bytes(752, 480, -1, 15) == -1 and L.aria_ray_algorithmic_bytes(752, 480, 65536, 15) == -1
    assert L.aria_ray_algorithmic_bytes(752, 480, 1, 16) == -1 and L.aria_ray_algorithmic_bytes(752, 480, 0, 15) == 0
    assert L.aria_ray_check(None) == -1


@pytest.mark.parametrize("field,value", [("struct_size", 0), ("nx", 12), ("ny", 0), ("nz", 1032), ("voxel", 0.0), ("voxel", float("nan")),
                                         ("min_weight", 0), ("min_weight", 65536), ("skip", 2), ("skip", -1), ("near", 0.0),
                                         ("near", float("nan")), ("near", 11.0), ("far", float("inf")), ("step", 0.0), ("step", -0.05),
                                         ("step", float("nan")), ("step", 0.001), ("fx", float("inf"))])
def test_ray_config_validation(aria, field, value):
    """A bad configuration is refused before any device is touched, and the restatement refuses the same. step = 0.001 asks
    for 9 701 samples."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    cfg = _lib.RayConfig()
    L.aria_ray_default_config(C.byref(cfg))
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert L.aria_ray_create(C.byref(cfg), C.byref(h)) == -1         # ARIA_E_INVALID
    assert not h.value
    assert L.aria_ray_create(None, C.byref(h)) == -1 and L.aria_ray_create(C.byref(cfg), None) == -1
    if field in ("nx", "ny", "nz"):
        dims = {"nx": 256, "ny": 256, "nz": 128}
        dims[field] = value
        with pytest.raises(ValueError):
            R.config(dims=(dims["nx"], dims["ny"], dims["nz"]))
    elif field not in ("struct_size", "fx"):
        with pytest.raises(ValueError):
            R.config(**{field: value})


def test_ray_n_steps_bounds(aria):
    """n_steps = (int)floorf((far - near) / step) + 1 in 1..8192: the bounds themselves pass validation (and then fail for
    the lack of a device here, or succeed), one beyond does not."""
    from aria_slam_amd import _lib
    L = aria.load_library()
    for near, far, step, steps in ((1.0, 8192.0, 1.0, 8192), (1.0, 8193.0, 1.0, None), (0.3, 0.3, 0.1, 1), (2.0, 2.6, 0.1, 6),
                                   (0.3, 10.0, 0.17, 58), (3.0, 10.0, 0.1, 71)):
        cfg = _lib.RayConfig()
        L.aria_ray_default_config(C.byref(cfg))
        cfg.near, cfg.far, cfg.step = near, far, step
        h = C.c_void_p()
        rc = L.aria_ray_create(C.byref(cfg), C.byref(h))
        if h.value:
            L.aria_ray_destroy(h)
        if steps is None:
            assert rc == -1
            with pytest.raises(ValueError):
                R.config(near=near, far=far, step=step)
        else:
            assert rc in (0, -2), (near, far, step, rc)
            assert R.n_steps(R.config(near=near, far=far, step=step)) == steps


def test_ray_calls_refuse_null_handles_and_bad_arguments(aria):
    L = aria.load_library()
    assert L.aria_ray_update_from_volume_device(None, None) == -1
    assert L.aria_ray_cast_batch_device(None, None, None, 1, 8, 8, None, 0, 8, None, 0, 8, None, 0, 8, None, 0, 8, None) == -1
    assert L.aria_ray_cast(None, None, 8, 8, None, None, None, None, None) == -1
    assert L.aria_ray_stream(None) is None
    L.aria_ray_destroy(None)


def test_no_gpu_means_ray_create_fails_loudly(aria):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(aria.AriaError) as e:
        aria.HipVolumeRenderer(dims=(8, 8, 8))
    assert e.value.status == -2                                      # ARIA_E_NO_DEVICE: there is no CPU fallback


# Measured with this restatement on the volume of TC.ref_scene() (voxel 0.1, step 0.1) at 80 x 60, per pose of TC.POSES:
# the fraction of pixels that hit; median and 95th percentile of |depth - truth| in metres over the pixels that hit; median
# and 95th percentile of the angle in degrees between the normal and (0, 0, -1) over the hit pixels whose truth is the
# plane, and the fraction of those that have a normal. Pose 0 is the grid-aligned view of the known limit.
# Rounded up to the digits shown; the table of DESIGN.md section 26 holds the same figures.
MEASURED = (dict(hit=0.9363, med=0.0245, p95=0.0479, nmed=0.48, np95=1.64, nfrac=0.974),
            dict(hit=0.8838, med=0.00056, p95=0.0500, nmed=0.42, np95=1.51, nfrac=0.934),
            dict(hit=0.8308, med=0.00059, p95=0.0629, nmed=0.48, np95=1.50, nfrac=0.933))


@pytest.mark.parametrize("i", range(3))
def test_ref_accuracy_on_the_analytic_scene(i):
    """The restatement against ground truth: depth against TC.render, plane normals against (0, 0, -1). Asserted: twice the
    measured median and 95th percentile per pose (the margin the volume's accuracy test uses), at least 0.8 of the pixels
    hit so that the statistics cannot hide a blank view, and at least 0.9 of the plane's hit pixels have a normal."""
    yaw, x = TC.POSES[i]
    c = RC.ref(RC.scene())[0][i]
    truth = TC.render(yaw, x)[0]
    plane = TC.render(yaw, x, sphere=False)[0]
    hit = c.depth > 0
    assert int(hit.sum()) == int(c.view["n_hit"])
    err = np.abs(c.depth.astype(np.float64) - truth)[hit & (truth > 0)]
    on_plane = hit & (truth > 0) & (truth == plane)
    n = c.normal[on_plane].astype(np.float64)
    has = np.linalg.norm(n, axis=1) > 0
    assert np.allclose(np.linalg.norm(n[has], axis=1), 1.0, atol=1e-6)
    ang = np.degrees(np.arccos(np.clip(-n[has][:, 2], -1.0, 1.0)))
    got = dict(hit=hit.mean(), med=np.median(err), p95=np.percentile(err, 95), nmed=np.median(ang), np95=np.percentile(ang, 95),
               nfrac=has.mean())
    print("pose %d: " % i + ", ".join("%s %.5f" % kv for kv in got.items()))
    m = MEASURED[i]
    assert got["hit"] >= 0.8 and got["nfrac"] >= 0.9
    assert got["med"] <= 2 * m["med"] and got["p95"] <= 2 * m["p95"]
    assert got["nmed"] <= 2 * m["nmed"] and got["np95"] <= 2 * m["np95"]
    assert 2 * m["p95"] < 1.5 * TC.VOXEL                             # the bounds themselves stay below a voxel and a half
    # the shade is the head-light term of the normal, recomputed here in fp64 from the normal and the pixel's ray
    u, v = np.meshgrid(np.arange(TC.W, dtype=np.float64), np.arange(TC.H, dtype=np.float64))
    dc = np.stack([(u - TC.K[2]) / TC.K[0], (v - TC.K[3]) / TC.K[1], np.ones_like(u)], axis=-1)
    d = dc @ TC.pose(yaw, x).reshape(3, 4)[:, :3]
    cos = np.abs((c.normal.astype(np.float64) * d).sum(-1)) / np.linalg.norm(d, axis=-1)
    assert np.abs(c.shade.astype(np.float64) - 255.0 * cos).max() <= 0.51
    assert not c.shade[~hit].any() and not c.gray[~hit].any() and not c.normal[~hit].any()


def _column(t_front, t_back, whole):
    """8 x 8 x 8 voxels of 1 m at the origin; the column (3, 3, *) -- or every column -- seen, t_front for z <= 3 and t_back
    behind; gray = 10 * z."""
    cfg = R.config(dims=(8, 8, 8), voxel=1.0, origin=(0, 0, 0), min_weight=2, near=0.5, far=9.5, step=1.0, K=(1, 1, 0, 0))
    vol = np.zeros((8, 8, 8), R.VOXEL_DTYPE)
    sel = (slice(None), slice(None), slice(None)) if whole else (slice(None), 3, 3)
    vol["weight"][sel] = 2
    vol["tsdf"][sel] = np.where(np.arange(8) <= 3, f32(t_front), f32(t_back)).reshape((8, 1, 1) if whole else (8,))
    vol["gray"][sel] = (10 * np.arange(8)).reshape((8, 1, 1) if whole else (8,))
    return cfg, vol


def test_ref_known_answer_single_column():
    """One pixel whose ray runs down the column (3, 3, *) from a camera at (3.5, 3.5, -2): sample k sits at the centre of voxel
    z = k - 2. tsdf +0.25 up to z = 3 and -0.75 behind: the walk ends at k = 6, the crossing lies 0.25 behind the centre
    z = 3.5 of voxel 3, at world z = 3.75, depth 5.75; alpha = 0.25 takes voxel 3's gray. With the column alone the cell of
    rule 6 is not defined: nearest-voxel values, no normal, shade 0. With every column filled alike the trilinear pair gives
    the same depth, the normal is (0, 0, -1) and the shade 255."""
    ext = TC.pose(x=3.5, y=3.5, z=-2.0)
    for whole in (False, True):
        cfg, vol = _column(0.25, -0.75, whole)
        st = {}
        c = R.cast(vol, cfg, ext, 1, 1, st)
        assert c.depth[0, 0] == f32(5.75) and c.gray[0, 0] == 30
        assert c.view.item() == (1, 1, f32(5.75), 1)
        if whole:
            assert st["trilinear"] == 1 and tuple(c.normal[0, 0]) == (0.0, 0.0, -1.0) and c.shade[0, 0] == 255
        else:
            assert st["nearest_voxel"] == 1 and not c.normal.any() and c.shade[0, 0] == 0
    # alpha = 0.5 takes the voxel behind (the extraction's rule)
    cfg, vol = _column(0.5, -0.5, False)
    c = R.cast(vol, cfg, ext, 1, 1)
    assert c.depth[0, 0] == f32(6.0) and c.gray[0, 0] == 40


def test_ref_known_answer_start_inside_and_back_face():
    """A ray that starts inside negative voxels ends at k = 0 without a hit: n_ended 1, n_hit 0, every plane 0. The same when
    the sample before the ending one is unseen (a back face of the seen region)."""
    cfg, vol = _column(0.5, -0.5, False)
    c = R.cast(vol, cfg, TC.pose(x=3.5, y=3.5, z=4.0), 1, 1)         # sample 0 at the centre of voxel z = 4
    assert c.view.item() == (0, 1, 0.0, 1) and c.depth[0, 0] == 0 and not c.normal.any() and c.gray[0, 0] == 0 and c.shade[0, 0] == 0
    vol = vol.copy()
    vol["weight"][3, 3, 3] = 1                                       # voxel 3 unseen: sample 5 is no sample
    c = R.cast(vol, cfg, TC.pose(x=3.5, y=3.5, z=-2.0), 1, 1)
    assert c.view.item() == (0, 1, 0.0, 1) and c.depth[0, 0] == 0
    # nothing negative on the ray: no walk ends
    vol["tsdf"] = 0.5
    c = R.cast(vol, cfg, TC.pose(x=3.5, y=3.5, z=-2.0), 1, 1)
    assert c.view.item() == (0, 0, 0.0, 1)


def test_ref_views_masked_and_non_finite():
    case = RC.scene()
    casts, invalid = RC.ref(case)
    assert invalid and casts[4] is None and [int(c.view["valid"]) for c in casts if c is not None] == [1, 1, 1, 1, 0]
    bad = casts[5]
    assert not bad.depth.any() and not bad.normal.any() and not bad.gray.any() and not bad.shade.any() and bad.view.tobytes() == bytes(16)
    masked, invalid = R.cast_batch(case.vol, case.cfg, case.ext, 8, 6, [1, 0, 0, 0, 0, 0])
    assert not invalid and [c is None for c in masked] == [False] + [True] * 5


def test_ref_cases_reach_every_branch():
    """What the device tests rely on, measured with this restatement: shape (b) has hits on both branches of rule 7 and of
    rule 9 in every 16 x 12 view; the clip cases hold what their names say."""
    for which in ("small", "many"):
        case = RC.small(which)
        total = dict(trilinear=0, nearest_voxel=0, normals=0, no_normal=0)
        for f in range(3):
            st = RC.ref_stats(case, f)
            assert 40 <= st["hits"] <= 80 and st["trilinear"] >= 1 and st["nearest_voxel"] >= 1 and st["normals"] >= 1
            for k in total:
                total[k] += st[k]
        assert min(total.values()) >= 1, (which, total)
    hits = {n: int(RC.ref(RC.frustum(n))[0][0].view["n_hit"]) for n in TC.FRUSTUM_POSES}
    assert hits == dict(inside=76, half_behind=0, outside=0, yaw_pitch=2624, narrow=292)
    seen_once = RC.ref(RC.half_behind_seen_once())[0][0].view
    assert int(seen_once["n_hit"]) == 0 and int(seen_once["n_ended"]) == 172
    assert int(RC.ref(RC.frustum("inside"))[0][0].view["n_ended"]) == 970
    want = dict(default=(195, 4242), odd_step=(58, 4107), short=(6, 2459), beyond=(71, 0), one=(1, 0))
    for n, (steps, n_hit) in want.items():
        case = RC.ranged(n)
        assert (R.n_steps(case.cfg), int(RC.ref(case)[0][0].view["n_hit"])) == (steps, n_hit), n
    assert [c.view.item() for c in RC.ref(RC.grazing())[0]] == [(1, 1, 5.75, 1), (0, 0, 0.0, 1), (1, 1, 5.75, 1), (0, 0, 0.0, 1)]
    views = [c.view for c in RC.ref(RC.slab())[0]]
    assert [int(v["n_hit"]) for v in views] == [2, 28, 12, 108] and [int(v["n_ended"]) for v in views] == [98, 36, 12, 108]


def test_pgm_writers_of_the_binding_round_trip(tmp_path):
    """The Python writers of the image formats euroc_frontend --render writes, and their reader."""
    from aria_slam_amd import render
    depth = np.array([[0.0, 0.3004, 1.2344], [65.6, 9.9996, np.float32(2.0005)]], np.float32)
    render.write_depth_pgm(str(tmp_path / "d.pgm"), depth)
    assert render.read_pgm(str(tmp_path / "d.pgm")).tolist() == [[0, 300, 1234], [65535, 10000, 2000]]
    shade = (np.arange(12, dtype=np.uint8) * 23).reshape(3, 4)
    render.write_gray_pgm(str(tmp_path / "s.pgm"), shade)
    assert (render.read_pgm(str(tmp_path / "s.pgm")) == shade).all()
