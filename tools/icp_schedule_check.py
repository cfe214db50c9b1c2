#!/usr/bin/env python3
"""The two schedules of k_icp_accumulate on the cases of tests/icp_cases.py: the shipped one (four pixels per lane) and the
plain one of the variants build (ARIA_ICP_SCHEDULE=plain, read when a handle is created: one pixel per lane, one atomic set per
wave) give the same 29 integers at every level and the same poses and records, bit for bit, and both equal the restatement.
ARIA_ORB_HIP_LIBRARY must name the variants build: the product library knows no switch and would run the shipped kernel twice,
so anything else is refused. Prints two lines per case and "icp schedules agree"."""
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
    for name in IC.SINGLES:
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
    print("icp schedules agree")


if __name__ == "__main__":
    main()
