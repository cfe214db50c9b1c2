"""Shared inputs of the ray casting tests (test_ray_host.py, test_ray_kernel_emulation.py, test_gpu_ray.py): the volumes of
tests/tsdf_cases.py under the views of shapes (a), (b) and (c), the guarded output layouts, and the restatement's results on
them (aria_slam_amd/ray_ref.py), computed once per process and handed out read-only.

A case is what one cast call gets: a volume, a ray_ref.Config, n views with an optional mask, and the view size. A runner
(the emulated kernels, the device) fills guarded buffers for a case, a layout and a set of planes; `expected` builds the
same buffers from the restatement, so one comparison of bytes checks the values, the masked view, the zeroed invalid view,
the padding and everything outside W x H."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as TC   # noqa: E402
from aria_slam_amd import ray_ref as RR   # noqa: E402

GUARD = TC.GUARD
PLANES = ("depth", "normal", "gray", "shade")
DTYPES = dict(depth=np.float32, normal=np.float32, gray=np.uint8, shade=np.uint8)
PER_PIXEL = dict(depth=1, normal=3, gray=1, shade=1)

Case = namedtuple("Case", "name vol cfg ext mask W H")

SCENE_POSES = TC.POSES + ((0.3, -0.5),)
SMALL_VIEW, SMALL_VIEW_K = (16, 12), (8.0, 8.0, 7.5, 5.5)
TINY_VIEW, TINY_VIEW_K = (TC.SMALL_W, TC.SMALL_H), TC.SMALL_K
RANGE_POSE = (0.15, -0.3)
RANGES = {                                                            # step, near, far
    "default": (0.05, 0.3, 10.0),                                     # 195 steps
    "odd_step": (0.17, 0.3, 10.0),                                    # 58 steps, not commensurate with the voxel
    "short": (0.1, 2.0, 2.6),                                         # 6 steps (fp32: floorf(0.6f / 0.1f) = 5)
    "beyond": (0.1, 3.0, 10.0),                                       # starts beyond the volume
    "one": (0.1, 0.3, 0.3),                                           # n_steps 1
}


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def scene():
    """Shape (a): the scene volume under the three TC.POSES and (yaw 0.3, x -0.5), then a masked view and one with an Inf
    extrinsic, 80 x 60."""
    tcfg, vol, _ = TC.ref_scene()
    ext = np.stack([TC.pose(yaw, x) for yaw, x in SCENE_POSES] + [TC.pose(0.1, 0.1), TC.pose(-0.1, 0.2)])
    ext[5, 7] = np.inf
    return Case("scene", vol, RR.from_tsdf(tcfg), _ro(ext), _ro(np.array([1, 1, 1, 9, 0, 1], np.uint8)), TC.W, TC.H)


def scene_single(i):
    """View i of shape (a) alone, unmasked."""
    c = scene()
    return Case("scene_%d" % i, c.vol, c.cfg, _ro(c.ext[i:i + 1]), None, c.W, c.H)


def small(which, tiny=False):
    """Shape (b): the 8 x 8 x 8 volumes `small` and `many` under the three poses of TC.small_frames(), 16 x 12 or 5 x 3."""
    tcfg, vol, _ = TC.ref_small() if which == "small" else TC.ref_many()
    (W, H), K = (TINY_VIEW, TINY_VIEW_K) if tiny else (SMALL_VIEW, SMALL_VIEW_K)
    cfg = RR.from_tsdf(tcfg, K=K, near=0.5, far=3.0, step=0.25)
    return Case("%s_%s" % (which, "tiny" if tiny else "view"), vol, cfg, TC.small_frames()[2], None, W, H)


def frustum(name):
    """Shape (c): the scene volume seen from a camera of TC.FRUSTUM_POSES."""
    tcfg, vol, _ = TC.ref_scene()
    (W, H), K = TC.frustum_view(name)
    return Case("frustum_" + name, vol, RR.from_tsdf(tcfg, K=K), _ro(TC.pose(**TC.FRUSTUM_POSES[name])[None]), None, W, H)


def ranged(name):
    """Shape (c): step and range variants at pose (0.15, -0.3)."""
    tcfg, vol, _ = TC.ref_scene()
    step, near, far = RANGES[name]
    return Case("range_" + name, vol, RR.from_tsdf(tcfg, step=step, near=near, far=far), _ro(TC.pose(*RANGE_POSE)[None]), None, TC.W, TC.H)


def half_behind_seen_once():
    """Shape (c), `half_behind` with min_weight = 1: the camera sits inside the sphere, whose far side one frame saw from
    within the truncation band, so walks end at a seen negative sample without a hit. (At the scene's own min_weight = 2 no
    such voxel is seen and n_ended is 0.)"""
    c = frustum("half_behind")
    return Case("frustum_half_behind_seen_once", c.vol, c.cfg._replace(min_weight=1), c.ext, None, c.W, c.H)


SLAB_DIMS, SLAB_VOXEL, SLAB_ORIGIN = (16, 8, 8), 0.25, (-2.0, -1.0, 0.5)
SLAB_POSES = (dict(), dict(yaw=0.6, x=-2.8, z=0.9), dict(yaw=-0.5, pitch=0.3, x=2.6, y=-0.9, z=0.7), dict(yaw=0.1, x=-0.4, z=1.1))


def slab():
    """A hand-filled volume whose walks end ON the box's faces, which the fused scenes never do (their border voxels are
    unseen), so that a clip range cut short by one sample at either end changes bytes: every voxel seen at +0.5; for x < 8 the
    first and the last z layer at -0.5 (a ray from the front ends at its first sample inside the box, a ray through a side
    face walks to a hit at its last); the brick x >= 8 holds one barely negative voxel, a zero, a minus zero and an unseen
    negative one. Views: from the front, through each x face, and from inside."""
    cfg = RR.config(dims=SLAB_DIMS, voxel=SLAB_VOXEL, origin=SLAB_ORIGIN, min_weight=2, near=0.3, far=4.0, step=0.25, K=SMALL_VIEW_K)
    vol = np.zeros(SLAB_DIMS[::-1], RR.VOXEL_DTYPE)
    vol["weight"], vol["tsdf"] = 2, 0.5
    vol["gray"] = (np.arange(vol.size) * 7 % 251).reshape(vol.shape)
    vol["tsdf"][0, :, :8] = -0.5
    vol["tsdf"][7, :, :8] = -0.5
    vol["tsdf"][5, 4, 12] = -0.001
    vol["tsdf"][2, 4, 13] = 0.0
    vol["tsdf"][3, 3, 10] = -0.0
    vol["tsdf"][1, 1, 9], vol["weight"][1, 1, 9] = -0.7, 1
    return Case("slab", _ro(vol), cfg, _ro(np.stack([TC.pose(**kw) for kw in SLAB_POSES])), None, *SMALL_VIEW)


def grazing():
    """Rays that run along a face of the box, where only the widened slabs of the clip keep them: 8 x 8 x 8 voxels of 1 m at
    the origin, every voxel seen, tsdf +0.25 up to z = 3 and -0.75 behind, one pixel on the optical axis. View 0: the camera
    on the face x = -0.5 of the box in grid units, the ray tilted outward by less than an ulp of its position, so that the
    computed g_x stays exactly -0.5 (rintf gives -0, inside) while the exact ray leaves the box at z = 0. View 1: the same on
    the face y = 7.5 (rintf(7.5) = 8 is outside: no hit, and the clip must not invent one). Views 2 and 3: |dg| of 1e-5 on x
    towards and away from the box from a camera one ulp outside and inside the face. The crossing lies at depth 5.75."""
    cfg = RR.config(dims=(8, 8, 8), voxel=1.0, origin=(0, 0, 0), min_weight=2, near=0.5, far=9.5, step=1.0, K=(1, 1, 0, 0))
    vol = np.zeros((8, 8, 8), RR.VOXEL_DTYPE)
    vol["weight"] = 2
    vol["tsdf"] = np.where(np.arange(8) <= 3, np.float32(0.25), np.float32(-0.75)).reshape(8, 1, 1)
    vol["gray"] = (10 * np.arange(8)).reshape(8, 1, 1)
    ext = np.stack([TC.pose(x=0.0, y=3.5, z=-2.0), TC.pose(x=3.5, y=8.0, z=-2.0), TC.pose(x=float(np.nextafter(np.float32(0), np.float32(-1))), y=3.5, z=-2.0),
                    TC.pose(x=float(np.nextafter(np.float32(0), np.float32(1))), y=3.5, z=-2.0)])
    ext[0, 8] = -1e-9                                                # r20: d_x = -1e-9
    ext[1, 9] = 1e-9                                                 # r21: d_y = +1e-9
    ext[2, 8], ext[3, 8] = 1e-5, -1e-5
    return Case("grazing", _ro(vol), cfg, _ro(ext), None, 1, 1)


def all_cases():
    """Shapes (a), (b) and (c), the slab and the grazing rays, by name."""
    out = [scene()] + [small(w, t) for w in ("small", "many") for t in (False, True)]
    out += [frustum(n) for n in sorted(TC.FRUSTUM_POSES)] + [ranged(n) for n in RANGES] + [half_behind_seen_once(), slab(), grazing()]
    return {c.name: c for c in out}


def ref(case):
    """(casts, invalid) of the restatement for a case, cached by the case's name; masked views are None."""
    def build():
        casts, invalid = RR.cast_batch(case.vol, case.cfg, case.ext, case.W, case.H, case.mask)
        for c in casts:
            for a in c or ():
                a.setflags(write=False)
        return casts, invalid
    return TC.ref("ray_" + case.name, build)


def ref_stats(case, view):
    """The branch counts of rules 7 and 9 for one view of a case."""
    st = {}
    RR.cast(case.vol, case.cfg, case.ext[view], case.W, case.H, st)
    return st


def dense_layout(W, H):
    """{plane: (pitch, stride)}: every plane dense."""
    return {p: (W, PER_PIXEL[p] * W * H) for p in PLANES}


def padded_layout(W, H):
    """Every plane with a pitch above the width and a stride above the view, all different."""
    return dict(depth=(W + 3, (W + 3) * H + 5), normal=(W + 2, 3 * (W + 2) * H + 7), gray=(W + 1, (W + 1) * H + 3),
                shade=(W + 5, (W + 5) * H + 1))


def guarded(case, layout, planes=PLANES):
    """{plane: [n_views, stride] of GUARD bytes} for the requested planes, and "views": n_views records of GUARD bytes."""
    n = len(case.ext)
    out = {p: np.full((n, layout[p][1] * np.dtype(DTYPES[p]).itemsize), GUARD, np.uint8).view(DTYPES[p]) for p in planes}
    out["views"] = np.full(n * RR.VIEW_DTYPE.itemsize, GUARD, np.uint8).view(RR.VIEW_DTYPE)
    return out


def expected(case, layout, planes=PLANES):
    """The buffers of `guarded` as the restatement fills them."""
    casts, _ = ref(case)
    out = guarded(case, layout, planes)
    for f, c in enumerate(casts):
        if c is None:
            continue
        out["views"][f] = c.view
        for p in planes:
            pitch, per = layout[p][0], PER_PIXEL[p]
            plane = getattr(c, p).reshape(case.H, case.W * per)
            for v in range(case.H):
                out[p][f, per * v * pitch: per * (v * pitch + case.W)] = plane[v]
    return out


def same_bytes(got, want):
    """The names of the buffers that differ, with the number of differing bytes."""
    return {k: int((np.frombuffer(got[k].tobytes(), np.uint8) != np.frombuffer(want[k].tobytes(), np.uint8)).sum())
            for k in want if got[k].tobytes() != want[k].tobytes()}
