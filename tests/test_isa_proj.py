"""The guided-matching kernels' gfx950 listing (aria_slam_amd/csrc/proj_search.hip, cross-compiled with the Makefile's flags; no
GPU): what the compiler's resource metadata and the instruction histogram of tools/isa_kernel_stats.py say about the promises
of the file's header -- no scratch, no floating-point atomic, every operation of the projection rounded once.

The only fused multiply-adds allowed are those inside the correctly rounded fp64 divisions of the projection (x / z and y / z).
The compiler's expansion of an fp64 division is a reciprocal refined by Newton steps and a residual correction, at most five
fused operations, and ends in one v_div_fixup_f64; so the fused count is held to five per v_div_fixup_f64, and a kernel without
a division may hold none."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

KERNELS = ("k_proj_bin", "k_proj_search", "k_proj_resolve", "k_proj_compact", "k_proj_from_map")


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
    path = os.path.join(out, "proj_search.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path,
                                                            os.path.join(csrc, "proj_search.hip")])
    return open(path).read()


def _kernel(listing, fragment):
    names = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S*%s\S*)" % re.escape(fragment), listing, re.M)))
    assert len(names) == 1, (fragment, names)
    return S.kernel_body(listing, names[0])


@pytest.mark.parametrize("k", KERNELS)
def test_proj_kernels_have_no_scratch_and_no_float_atomics(listing, k):
    body, meta = _kernel(listing, k)
    assert len(body) > 5, k
    assert meta.get("ScratchSize", -1) == 0, (k, meta)
    hist, _, _ = S.stats(body)
    assert not any(op.startswith(("global_atomic", "buffer_atomic", "flat_atomic", "ds_")) and ("f32" in op or "f64" in op)
                   and ("add" in op or "min" in op or "max" in op) for op in hist), (k, hist)


@pytest.mark.parametrize("k", KERNELS)
def test_proj_kernels_fuse_nothing_outside_the_divisions(listing, k):
    body, _ = _kernel(listing, k)
    hist, _, _ = S.stats(body)
    assert not any(op.startswith(("v_fma_f32", "v_fmac_f32", "v_fma_mix", "v_mad_f32", "v_mac_f32", "v_pk_fma")) for op in hist), (k, hist)
    fused64 = sum(n for op, n in hist.items() if op.startswith(("v_fma_f64", "v_fmac_f64")))
    divisions = hist.get("v_div_fixup_f64", 0)
    assert fused64 <= 5 * divisions, (k, fused64, divisions)
    if k == "k_proj_search":
        assert divisions == 2, hist                                   # x / z and y / z of the projection, nothing else
    else:
        assert divisions == 0 and fused64 == 0, (k, hist)
