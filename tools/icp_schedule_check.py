#!/usr/bin/env python3
"""The two schedules of k_icp_accumulate on the cases of tests/icp_cases.py: the shipped one (four pixels per lane) and the
plain one of the variants build (ARIA_ICP_SCHEDULE=plain, read when a handle is created: one pixel per lane, one atomic set per
wave) give the same 29 integers at every level and the same poses and records, bit for bit, and both equal the restatement.
ARIA_ORB_HIP_LIBRARY must name the variants build: the product library knows no switch and would run the shipped kernel twice,
so anything else is refused. Prints two lines per case and "icp schedules agree". With --tables it runs the hand-written rule
table and solve table of tests/icp_cases.py instead of the named cases (tests/test_gpu_icp_rules.py does), two lines per
table entry, worded differently: the callers count lines."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import aria_slam_amd as A
    import icp_cases as IC
    from aria_slam_amd import icp_ref as IR
    assert A.library_path().endswith("libaria_orb_hip_variants.so"), "set ARIA_ORB_HIP_LIBRARY to the variants build"
    assert torch.cuda.is_available()
    dev = lambda a: torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to("cuda:0")   # noqa: E731
    tables = "--tables" in sys.argv[1:]
    for name in () if tables else IC.SINGLES:
        f = IC.frame(name)
        cfg = IC.config(f.K)
        b = IC.batch([name])
        want = IC.expected(b, cfg)
        trel = IR.relative(f.Tm, f.T0)
        d = {k: dev(v) for k, v in IC.pack(b, IC.layout(f.W, f.H)).items()}
        d_trel = dev(np.array(trel))
        torch.cuda.synchronize()
        for sched in ("shipped", "plain"):
            if sched == "plain":
                os.environ["ARIA_ICP_SCHEDULE"] = "plain"
            h = A.HipDenseTracker.from_ref_config(cfg)
            os.environ.pop("ARIA_ICP_SCHEDULE", None)
            gp, gr = IC.guarded_outputs(1)
            dp, dr = dev(gp), dev(gr)
            d_sys = dev(np.zeros(IR.N_TERMS, np.int64))
            torch.cuda.synchronize()
            diff = 0
            for stride in cfg.strides:
                h.debug_system(d["live"], d["depth"], d["normal"], d["Tm"], d_trel, 1, f.W, f.H, stride, d_sys)
                h.check()
                got = d_sys.cpu().numpy().view(np.int64)
                diff += int((got != IR.system(cfg, f.D, f.M, f.N, trel, IR.model_rotation(f.Tm), stride)).sum())
            h.track_batch_device(d["live"], d["depth"], d["normal"], d["Tm"], d["T0"], 1, f.W, f.H, d_extrinsics_out=dp, d_results=dr)
            h.check()
            h.close()
            p, r = dp.cpu().numpy().tobytes(), dr.cpu().numpy().tobytes()
            nbytes = sum(x != y for x, y in zip(p + r, want[0].tobytes() + want[1].tobytes()))
            print("%s %s: %d bytes of pose and record and %d integers differ from the restatement" % (name, sched, nbytes, diff))
            assert nbytes == 0 and diff == 0, (name, sched)

    def handle(cfg, sched):
        if sched == "plain":
            os.environ["ARIA_ICP_SCHEDULE"] = "plain"
        h = A.HipDenseTracker.from_ref_config(cfg)
        os.environ.pop("ARIA_ICP_SCHEDULE", None)
        return h

    # the hand-written tables (rule 3 test by test, rule 5 pivot by pivot), on lines of their own
    for g in IC.rule_cases() if tables else ():
        n = len(g.batch.frames)
        d = {k: dev(v) for k, v in IC.pack(g.batch, IC.layout(g.batch.W, g.batch.H)).items()}
        d_trel, d_sys = dev(np.array(g.trels)), dev(np.zeros((n, IR.N_TERMS), np.int64))
        torch.cuda.synchronize()
        for sched in ("shipped", "plain"):
            h = handle(g.cfg, sched)
            diff = 0
            for stride in (1, 2):
                h.debug_system(d["live"], d["depth"], d["normal"], d["Tm"], d_trel, n, g.batch.W, g.batch.H, stride, d_sys)
                h.check()
                diff += int((d_sys.cpu().numpy().view(np.int64).reshape(n, IR.N_TERMS) != IC.rule_systems(g, stride)).sum())
            h.close()
            print("rule table %s, %s schedule, %d frames: integers that differ from the restatement: %d" % (g.name, sched, n, diff))
            assert diff == 0, (g.name, sched)
    for c in IC.solve_cases() if tables else ():
        f = c.frame
        want = IC.solve_ref(c)[0]
        d = {k: dev(v) for k, v in IC.pack(IC.Batch([f], None, f.W, f.H, f.K), IC.layout(f.W, f.H)).items()}
        torch.cuda.synchronize()
        for sched in ("shipped", "plain"):
            h = handle(c.cfg, sched)
            gp, gr = IC.guarded_outputs(1)
            dp, dr = dev(gp), dev(gr)
            torch.cuda.synchronize()
            h.track_batch_device(d["live"], d["depth"], d["normal"], d["Tm"], d["T0"], 1, f.W, f.H, d_extrinsics_out=dp, d_results=dr)
            h.check()
            h.close()
            got = dp.cpu().numpy().tobytes() + dr.cpu().numpy().tobytes()
            nbytes = sum(x != y for x, y in zip(got, want.T.tobytes() + want.result.tobytes()))
            print("solve table %s, %s schedule: differing bytes of pose and record: %d" % (c.name, sched, nbytes))
            assert nbytes == 0, (c.name, sched)
    print("icp schedules agree")


if __name__ == "__main__":
    main()
