"""The tracking kernels' gfx950 listing (aria_slam_amd/csrc/icp_track.hip, cross-compiled with the Makefile's flags; no GPU):
what the compiler's resource metadata and the instruction histogram of tools/isa_kernel_stats.py say about the promises of
the file's header.

Occupancy: k_icp_accumulate keeps 28 fp64 partial sums (56 VGPRs) beside the pixel's own values, so it is built for 4 waves
per SIMD, which on gfx950 (512 VGPRs per SIMD lane) means at most 128 VGPRs. The kernel is bound by its fp64 arithmetic and
the gathers of a 16 x 4 tile, not by latency that more waves would hide. k_icp_solve is one lane per frame and its
occupancy does not matter; it only has to stay out of scratch."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

ACCUMULATE = "k_icp_accumulateILi4EE"                                  # the shipped schedule: four pixels per lane
SOLVE = "k_icp_solve"


@pytest.fixture(scope="module")
def listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS := (.*?)(?<!\\)$", mk, re.M | re.S).group(1).replace("\\\n", " ").split()
    for f in ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-O3"):
        assert f in flags, f
    flags = [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", ROOT) for f in flags if f != "-shared"]
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "icp_track.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path,
                                                            os.path.join(csrc, "icp_track.hip")])
    return open(path).read()


def _kernel(listing, fragment):
    names = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S*%s\S*)" % re.escape(fragment), listing, re.M)))
    assert len(names) == 1, (fragment, names)
    return S.kernel_body(listing, names[0])


def test_icp_kernels_have_no_scratch_and_no_float_atomics(listing):
    for k in (ACCUMULATE, SOLVE):
        body, meta = _kernel(listing, k)
        assert len(body) > 5, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        hist, _, _ = S.stats(body)
        assert not any(op.startswith(("global_atomic", "buffer_atomic", "flat_atomic")) and ("f32" in op or "f64" in op) for op in hist), k


def test_icp_accumulate_rounds_every_operation_once_at_four_waves_per_simd(listing):
    """k_icp_accumulate: at most 128 VGPRs (4 waves per SIMD) and no fused multiply-add outside the one correctly rounded
    division of a pixel (1.0f / q_z; its sequence holds at most 5) and the 28 double -> int64 conversions of the commit."""
    body, meta = _kernel(listing, ACCUMULATE)
    hist, _, _ = S.stats(body)
    assert 0 < meta.get("NumVgprs", meta.get("VGPRs", 999)) <= 128, meta
    assert not any(op.startswith(("v_fma_mix", "v_mad_f32", "v_mac_f32", "v_pk_fma")) for op in hist), hist
    # fp64: the only fused operation is the exact x - hi * 2^32 inside each double -> int64 conversion of the wave's commit
    fused64 = sum(n for op, n in hist.items() if op.startswith(("v_fma_f64", "v_fmac_f64")))
    to_int64 = sum(n for op, n in hist.items() if op.startswith("v_cvt_u32_f64"))
    assert fused64 == to_int64 <= 28, (fused64, to_int64)
    divisions = hist.get("v_div_fixup_f32", 0)
    fused = sum(n for op, n in hist.items() if op.startswith(("v_fma_f32", "v_fmac_f32")))
    assert divisions >= 1 and fused <= 5 * divisions, (fused, divisions)
