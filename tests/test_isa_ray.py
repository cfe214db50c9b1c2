"""The ray casting kernels' gfx950 listing (aria_slam_amd/csrc/tsdf_raycast.hip, cross-compiled with the Makefile's flags; no
GPU): what the compiler's resource metadata and the instruction histogram of tools/isa_kernel_stats.py say about the
promises of the file's header."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

KERNELS = ("k_ray_prepare", "k_ray_bricks", "k_ray_brick_words", "k_ray_march", "k_ray_finish")


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
    path = os.path.join(out, "tsdf_raycast.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path,
                                                            os.path.join(csrc, "tsdf_raycast.hip")])
    return open(path).read()


def test_ray_kernels_have_no_scratch_and_no_float_atomics(listing):
    for k in KERNELS:
        body, meta = S.kernel_body(listing, k)
        assert len(body) > 5, k
        assert meta.get("ScratchSize", -1) == 0, (k, meta)
        hist, _, _ = S.stats(body)
        assert not any(op.startswith(("global_atomic", "buffer_atomic", "flat_atomic")) and ("f32" in op or "f64" in op) for op in hist), k
        assert not any(op.startswith(("scratch_", "buffer_store", "buffer_load")) for op in hist), k


def test_ray_march_walks_in_registers_at_full_occupancy(listing):
    """k_ray_march: no LDS, no barrier, at most 64 VGPRs (8 waves per SIMD), the view record through scalar loads, the records
    as 8-byte gathers, integer atomics only for the view record, correctly rounded divisions and square roots, and no fused
    multiply-add anywhere."""
    body, meta = S.kernel_body(listing, "k_ray_march")
    hist, _, _ = S.stats(body)
    assert meta.get("LDSByteSize", -1) == 0 and "s_barrier" not in hist and not any(op.startswith("ds_") and "swizzle" not in op and "permute" not in op for op in hist)
    assert 0 < meta.get("NumVgprs", meta.get("VGPRs", 999)) <= 64, meta
    assert sum(n for op, n in hist.items() if op.startswith("s_load_dword")) >= 3
    records = hist.get("global_load_dwordx2", 0) + 2 * hist.get("global_load_dwordx4", 0)
    assert records >= 26, hist                                       # the walk, sample k - 1, three cells of eight (8 bytes each)
    atomics = {op for op in hist if op.startswith("global_atomic")}
    assert atomics and all(re.match(r"global_atomic_(add|umin|smin|min_u32|add_u32)", op) for op in atomics), atomics
    divisions = hist.get("v_div_fixup_f32", 0)
    roots = sum(n for op, n in hist.items() if op.startswith("v_sqrt_f32"))
    assert divisions >= 5 and roots >= 2                             # alpha, three normal components, the cosine; len and dl
    # the only fused multiply-adds are those inside the division and square root sequences (at most 5 and 3 each)
    assert not any(op.startswith(("v_fma_mix", "v_mad_f32", "v_mac_f32", "v_pk_fma")) for op in hist)
    fused = sum(n for op, n in hist.items() if op.startswith(("v_fma_f32", "v_fmac_f32")))
    assert fused <= 5 * divisions + 3 * roots, (fused, divisions, roots)


def test_ray_bricks_needs_no_atomic(listing):
    """The brick kernels: a run of eight records per lane, a plain byte store, no atomic of any kind, no LDS, no barrier."""
    for k in ("k_ray_bricks", "k_ray_brick_words"):
        body, meta = S.kernel_body(listing, k)
        hist, _, _ = S.stats(body)
        assert meta.get("LDSByteSize", -1) == 0 and "s_barrier" not in hist
        assert not any("atomic" in op for op in hist), k
    hist, _, _ = S.stats(S.kernel_body(listing, "k_ray_bricks")[0])
    loaded = sum(n * {"global_load_dwordx2": 1, "global_load_dwordx4": 2}.get(op, 0) for op, n in hist.items())
    assert loaded >= 8 and hist.get("global_store_byte", 0) >= 1


def test_tsdf_raycast_is_in_the_product_build_and_reads_no_environment():
    mk = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "Makefile")).read()
    src_line = [ln for ln in mk.splitlines() if ln.startswith("SRC :=")][0]
    assert "tsdf_raycast.hip" in src_line
    src = open(os.path.join(ROOT, "aria_slam_amd", "csrc", "tsdf_raycast.hip")).read()
    assert "getenv" not in src and "asm" not in src.replace("aria_slam_amd", "")
