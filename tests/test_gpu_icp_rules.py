"""Frame-to-model tracking on the MI355X on what the rendered scenes of tests/test_gpu_icp.py cannot ask: every test of rule 3
as the first to reject a pixel, every inclusive limit at equality and one ulp beyond, rintf on exact ties, non-finite inputs,
terms near the top of rule 4's proof, every pivot index of rule 5, the second workgroup of the per-frame kernels and the
largest image sizes. The cases are those of tests/icp_cases.py (rule_cases, solve_cases, batch300, strip_case);
tests/test_icp_rules_host.py shows on the restatement alone that they ask what they are named for. Every comparison is
bytes against aria_slam_amd/icp_ref.py: a difference is a bug, never a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC   # noqa: E402
from aria_slam_amd import icp_ref as IR   # noqa: E402
from test_gpu_icp import ARIA_E_INVALID, ROOT, Device, _handle, torch_cuda, work   # noqa: E402,F401  (the last two are fixtures)


def _single(f):
    return IC.Batch([f], None, f.W, f.H, f.K)


@pytest.mark.parametrize("padded", (False, True), ids=("dense", "padded"))
@pytest.mark.parametrize("group", (0, 1), ids=("even", "odd"))
def test_rule_table_equals_the_restatements_integers(torch_cuda, work, aria, group, padded):
    """Every frame of a group in one call, each at its own Trel. Padded: the live map's padding holds a valid depth, as `edge`."""
    g = IC.rule_cases()[group]
    d = Device(torch_cuda, work, g.batch, IC.layout(g.batch.W, g.batch.H, padded), live_fill=1.0 if padded else None)
    h = _handle(aria, work, g.cfg)
    try:
        for stride in (1, 2):
            got, want = d.system(h, g.trels, stride), IC.rule_systems(g, stride)
            for i, f in enumerate(g.batch.frames):
                print("%s stride %d: %d correspondences, differing terms %d" % (f.name, stride, int(want[i][28]), int((got[i] != want[i]).sum())))
            assert got.tobytes() == want.tobytes(), [f.name for i, f in enumerate(g.batch.frames) if (got[i] != want[i]).any()]
        assert d.inputs_intact()
    finally:
        h.close()


def test_bound_case_terms_near_the_top_of_the_proof(torch_cuda, work, aria):
    cfg, D, M, N, trel, Rm = IC.bound_case()
    f = IC.Frame("bound", D, M, N, IC.IDENTITY, IC.IDENTITY, IC.IDENTITY, 4, 4, cfg.K)
    d = Device(torch_cuda, work, _single(f), IC.layout(4, 4))
    h = _handle(aria, work, cfg)
    try:
        want = IR.system(cfg, D, M, N, trel, Rm, 1)
        got = d.system(h, [trel], 1)
        print("bound: %d correspondences, largest sum 2^%.2f, differing terms %d" %
              (int(want[28]), np.log2(float(np.abs(want[:28]).max())), int((got[0] != want).sum())))
        assert got[0].tobytes() == want.tobytes() and want[28] >= 8 and np.abs(want[:21]).max() > 2.0 ** 37
    finally:
        h.close()


@pytest.mark.parametrize("case", IC.solve_cases(), ids=[c.name for c in IC.solve_cases()])
def test_solve_table_poses_and_records(torch_cuda, work, aria, case):
    b = _single(case.frame)
    d = Device(torch_cuda, work, b, IC.layout(b.W, b.H))
    h = _handle(aria, work, case.cfg)
    try:
        assert h.ref_config == case.cfg                               # min_pivot to the last bit
        poses, recs, status = d.track(h)
        want = IC.solve_ref(case)[0]
        print(case.name, recs[0], "pose bytes differ: %d" % int((poses[0].view(np.uint8) != want.T.view(np.uint8)).sum()))
        assert status == 0 and recs[0].tobytes() == want.result.tobytes(), (recs[0], want.result)
        assert poses[0].tobytes() == want.T.tobytes()
    finally:
        h.close()


def test_batch_of_300_runs_the_second_workgroup_of_the_per_frame_kernels(torch_cuda, work, aria):
    """300 guesses for one 16 x 12 frame in one call: lost frames, masked frames on both sides of index 256 and a non-finite T0
    past it. Poses, records, the guard bytes of what must not be written, and ARIA_E_INVALID reported once."""
    cfg, b = IC.batch300()
    d = Device(torch_cuda, work, b, IC.layout(b.W, b.H))
    h = _handle(aria, work, cfg)
    try:
        poses, recs, status = d.track(h)
        want = IC.expected(b, cfg)
        bad = [i for i in range(IC.BIG_N) if poses[i].tobytes() != want[0][i].tobytes() or recs[i:i + 1].tobytes() != want[1][i:i + 1].tobytes()]
        print("batch of 300: %d valid, frames that differ: %s" % (int((want[1]["valid"] == 1).sum()), bad))
        assert want[2] and status == ARIA_E_INVALID and h.status() == 0       # reported once
        assert recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
        gp, gr = IC.guarded_outputs(IC.BIG_N)
        for i in IC.BIG_MASKED:
            assert poses[i].tobytes() == gp[i].tobytes() and recs[i:i + 1].tobytes() == gr[i:i + 1].tobytes()
        assert recs[IC.BIG_NAN:IC.BIG_NAN + 1].tobytes() == bytes(32) and poses[IC.BIG_NAN].tobytes() == gp[IC.BIG_NAN].tobytes()
        assert d.inputs_intact()
    finally:
        h.close()


@pytest.mark.parametrize("w,h_", ((IC.STRIP, 1), (1, IC.STRIP)), ids=("16384x1", "1x16384"))
def test_strips_at_the_size_limit(torch_cuda, work, aria, w, h_):
    """The 16384 of icp_bad_size: (float)u up to 16383, 1024 tiles across or 256 workgroups down, at strides 1 and 16; one track."""
    cfg, f, trel = IC.strip_case(w, h_)
    b = _single(f)
    d = Device(torch_cuda, work, b, IC.layout(w, h_))
    h = _handle(aria, work, cfg)
    try:
        for stride in (1, 16):
            want = IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)
            got = d.system(h, [trel], stride)
            print("%d x %d stride %d: %d correspondences, differing terms %d" % (w, h_, stride, int(want[28]), int((got[0] != want).sum())))
            assert got[0].tobytes() == want.tobytes() and 2 * int(want[28]) > IC.STRIP // stride
        poses, recs, status = d.track(h)
        want = IC.expected(b, cfg)
        assert status == 0 and recs.tobytes() == want[1].tobytes() and poses.tobytes() == want[0].tobytes()
        assert int(recs[0]["iterations_run"]) >= 2 and d.inputs_intact()
    finally:
        h.close()


def test_plain_schedule_of_the_variants_build_equals_the_restatement_on_the_tables(aria):
    """The rule table and the solve table through one pixel per lane and one atomic set per wave (ARIA_ICP_SCHEDULE=plain,
    variants build only), as test_gpu_icp.py does for the named cases: tools/icp_schedule_check.py --tables in a subprocess."""
    e = dict(os.environ)
    e["ARIA_ORB_HIP_LIBRARY"] = aria.build_variants_library()
    e.pop("ARIA_ICP_SCHEDULE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "icp_schedule_check.py"), "--tables"], env=e, capture_output=True,
                         text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    for sched in ("shipped", "plain"):
        assert out.stdout.count("%s schedule, " % sched) == len(IC.rule_cases()) and out.stdout.count("%s schedule: " % sched) == len(IC.solve_cases())
    assert out.stdout.count("differ from the restatement: 0\n") == 2 * len(IC.rule_cases())
    assert out.stdout.count("of pose and record: 0\n") == 2 * len(IC.solve_cases()) and "icp schedules agree" in out.stdout


def test_host_form_on_one_handle_small_large_small(torch_cuda, work, aria):
    """8 x 8, then 61 x 45, then 8 x 8 again on one handle: the staging buffers only grow, and each call equals the restatement."""
    cfg = IC.config(IC.KO)
    h = _handle(aria, work, cfg)
    try:
        for name in ("tiny", "odd", "tiny"):
            f = IC.frame(name)
            T0 = IC.SOLVE_T0 if name == "tiny" else f.T0              # a guess that is not Tm, so a lost frame's pose shows which was read
            want = IR.track(cfg, f.D, f.M, f.N, f.Tm, T0)
            t = h.track(f.D, f.M, f.N, f.Tm, T0)
            print(name, t.result)
            assert t.result.tobytes() == want.result.tobytes() and t.T.tobytes() == want.T.tobytes(), name
        assert int(want.result["n_corr"]) < 64                       # 8 x 8 after 61 x 45: nothing of the larger frame is counted
    finally:
        h.close()
