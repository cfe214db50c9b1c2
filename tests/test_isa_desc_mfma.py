"""Build-time check of the batch k_describe's matrix-core moment phase in the device ISA (CPU: hipcc cross-compiles gfx950
without a GPU).

describe16<0> (aria_slam_amd/csrc/orb_kernels.hip) computes the intensity-centroid moments of a wave's 16 keypoints as one int8
matrix product: 16 accumulating v_mfma_i32_16x16x64_i8, whose A operand is 16 pieces of the raw window per lane, each loaded
as a global_load_dwordx4 plus a global_load_dword and cut out with v_alignbyte. What the phase is for shows only in the
listing: the loads have to stay whole (a type of alignment 1, not split into bytes), the weights come from LDS as 16 ds_read_b128, the LDS realignment reads of the old rounds are gone,
and the kernel still fits four waves per SIMD without scratch."""
import collections
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402

CSRC = os.path.join(ROOT, "aria_slam_amd", "csrc")
# the flags of aria_slam_amd/csrc/Makefile (product build), device side only, to assembly
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-fno-fast-math", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--cuda-device-only", "-S", "-w"]
KERNEL = "k_describeILi0ELb1ELb1E"          # k_describe<0, true, true>
ARENA = "k_describeILi1ELb1ELb1E"           # k_describe<1, true, true>
MFMA = "v_mfma_i32_16x16x64_i8"
SUB_DWORD_LOADS = ("global_load_ubyte", "global_load_sbyte", "global_load_ushort", "global_load_sshort", "global_load_short_d16",
                   "global_load_ubyte_d16", "global_load_sbyte_d16")


def _listing(extra=()):
    src = os.path.join(CSRC, "orb_kernels.hip")
    h = hashlib.sha256(" ".join(extra).encode())
    for f in [src] + [os.path.join(CSRC, x) for x in ("common.h", "orb_device.h", "orb_kernels.h", "orb_plan.h", "ic_moment_weights.h")]:
        h.update(open(f, "rb").read())
    out_dir = os.path.join(ROOT, "build", "isa")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "orb_kernels.hip.desc.%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + list(extra) + ["-o", out, src])
    return open(out).read()


def _hist(text, kernel):
    body, meta = S.kernel_body(text, kernel)
    assert len(body) > 200, "kernel %s not found in the listing" % kernel
    return body, collections.Counter(ln.split()[0] for ln in body), meta


@pytest.fixture(scope="module")
def product_listing():
    return _listing()


def test_moment_phase_is_sixteen_mfma_on_whole_loads(product_listing):
    body, hist, meta = _hist(product_listing, KERNEL)
    print(KERNEL, meta, {k: v for k, v in hist.items() if k.startswith(("v_mfma", "global_load", "ds_read", "ds_write"))})
    assert hist[MFMA] == 16 and sum(v for k, v in hist.items() if k.startswith("v_mfma")) == 16
    assert not [k for k in hist if k.startswith(SUB_DWORD_LOADS)], "a window load was split into sub-dword loads"
    # the phase between its first and last MFMA: the second half of the window (8 pieces) is requested inside it, the first
    # half just in front of it; nothing else in the kernel loads 16 bytes before the first MFMA but the weight piece
    at = [i for i, ln in enumerate(body) if ln.startswith(MFMA)]
    before = sum(1 for ln in body[:at[0]] if ln.startswith("global_load_dwordx4"))
    inside = sum(1 for ln in body[at[0]:at[-1] + 1] if ln.startswith("global_load_dwordx4"))
    assert before + inside >= 1 + 16 and before >= 1 + 8, (before, inside)
    # each piece is cut out of five dwords from the dword-aligned start with four v_alignbyte; the fifth dword comes from the
    # neighbouring lane, and is loaded only in the seven steps whose rows reach it inside the disc
    assert hist["global_load_dword"] == 7 and hist["v_alignbyte_b32"] == 64, hist
    # weights: 16 ds_read_b128; no dword reads of a realigned window (the old rounds read 32 per round)
    assert hist["ds_read_b128"] == 16 and hist["ds_read_b32"] == 0 and hist["ds_read2_b32"] == 0, hist
    # one row_shl:4 brings m01 to the keypoint's lane
    assert sum(1 for ln in body if "row_shl:4" in ln) == 1


def test_batch_kernel_keeps_four_waves_without_scratch(product_listing):
    _, _, meta = _hist(product_listing, KERNEL)
    assert meta.get("TotalNumVgprs", 999) <= 128 and meta.get("Occupancy") == 4 and meta.get("ScratchSize", 1) == 0, meta
    in_loop, outside = S.scratch_accesses(product_listing, KERNEL)
    assert not in_loop and not outside


def test_mfma_beside_packed_fp32_has_no_crossed_half(product_listing):
    """The kernel's own MFMAs now share the SIMD with its v_pk_*_f32 (tests/test_isa_lint.py: the round-3 hazard form)."""
    body, _, _ = _hist(product_listing, KERNEL)
    crossed, _ = S.swizzled_pk_f32(body)
    assert not crossed, "\n".join(crossed[:8])


def test_arena_kernel_keeps_the_lds_rounds(product_listing):
    _, hist, _ = _hist(product_listing, ARENA)
    assert not [k for k in hist if k.startswith("v_mfma")]


def test_lds_moment_build_is_the_old_rounds():
    """-DARIA_DESC_MOMENTS_LDS=1 (the A side of A/B measurements, tools/build_ab.sh): no MFMA, the window goes through LDS."""
    text = _listing(("-DARIA_DESC_MOMENTS_LDS=1",))
    _, hist, meta = _hist(text, KERNEL)
    assert not [k for k in hist if k.startswith("v_mfma")]
    assert hist["ds_write_b128"] >= 7 and hist["v_dot4_u32_u8"] >= 32, hist
    assert meta.get("TotalNumVgprs", 999) <= 128 and meta.get("Occupancy") == 4 and meta.get("ScratchSize", 1) == 0, meta
