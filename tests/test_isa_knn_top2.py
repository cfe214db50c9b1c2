"""Build-time check of the matcher's running top-2 in the device ISA (CPU: hipcc cross-compiles gfx950 without a GPU).

The matrix-core kNN-2 kernels (aria_slam_amd/csrc/knn2_mfma.hip) are bound by vector-instruction issue, and the running top-2
is most of their vector work. The grouped update (top2_quad) takes 5 three-input instructions (v_med3_f32 / v_min3_i32) per 4
keys where the per-distance form took 8. An accumulator of 16 keys is produced by 4 FP4 MFMAs or by 8 int8 MFMAs, so the tile
loop holds
    FP4  (k_knn2_fp4):   16 * 1.25 / 4 = 5.0 three-input instructions per MFMA   (per-distance form: 8.0)
    int8 (k_knn2_mfma):  16 * 1.25 / 8 = 2.5                                      (per-distance form: 4.0)
Both are held with 10 % of slack for what the compiler may add around the update: 5.5 and 2.75.

The count is taken twice: over the instructions between the first and the last MFMA of the kernel (the updates of the last
accumulator pair of a loop trip come after its last MFMA, so this span sees 3.75 / 1.875 per MFMA, 6.0 / 3.0 in the
per-distance form), and over the whole tile loop (every basic block the listing marks as part of a loop), which sees all of
them. Neither span may touch scratch memory: what the allocator spills has to stay outside the loop."""
import hashlib
import os
import re
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
THREE_INPUT = re.compile(r"^v_(min3|med3|max3)_")


def _listing(extra=()):
    src = os.path.join(CSRC, "knn2_mfma.hip")
    h = hashlib.sha256(" ".join(extra).encode())
    for f in [src] + [os.path.join(CSRC, x) for x in ("common.h", "match_kernels.h")]:
        h.update(open(f, "rb").read())
    out_dir = os.path.join(ROOT, "build", "isa")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "knn2_mfma.hip.%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + list(extra) + ["-o", out, src])
    return open(out).read()


@pytest.fixture(scope="module")
def product_listing():
    return _listing()


def _loop_instructions(text, name_sub):
    """Instructions of every basic block of the kernel that LLVM's listing marks as part of a loop (as S.scratch_accesses)."""
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines)
                 if ln.split(";")[0].strip().endswith(":") and name_sub in ln.split(";")[0] and not ln.startswith(("\t", ".L")))
    out, looping = [], False
    for ln in lines[start + 1:]:
        t = ln.strip()
        if t.startswith(".section") or t.startswith(".amdhsa_kernel"):
            break
        if t.startswith(".LBB") or t.startswith("; %bb."):
            looping = "Loop" in t
        elif looping and t and not t.startswith((";", ".")):
            out.append(t.split(";")[0].strip())
    return out


def _counts(text, kernel):
    body, meta = S.kernel_body(text, kernel)
    assert len(body) > 200, "kernel %s not found in the listing" % kernel
    at = [i for i, ln in enumerate(body) if ln.startswith("v_mfma")]
    span = body[at[0]:at[-1] + 1]
    loop = _loop_instructions(text, kernel)
    n_loop_mfma = sum(1 for ln in loop if ln.startswith("v_mfma"))
    assert n_loop_mfma == len(at), "every MFMA of %s belongs to the tile loop (%d of %d)" % (kernel, n_loop_mfma, len(at))
    return {"mfma": len(at), "span3": sum(1 for ln in span if THREE_INPUT.match(ln)),
            "loop3": sum(1 for ln in loop if THREE_INPUT.match(ln)),
            "scratch": [ln for ln in span + loop if ln.startswith("scratch_")], "meta": meta}


# kernel (mangled-name piece), MFMAs per 32 x 32 accumulator
KERNELS = [("k_knn2_fp4ILi0ELi4ELi64E", 4), ("k_knn2_mfmaILi0ELb0ELi4ELi64E", 8)]


@pytest.mark.parametrize("kernel,mfma_per_acc", KERNELS)
def test_grouped_top2_instruction_count(product_listing, kernel, mfma_per_acc):
    c = _counts(product_listing, kernel)
    bound = 1.1 * 16 * 1.25 / mfma_per_acc                  # 5.5 (FP4) / 2.75 (int8), see the module docstring
    per_span, per_loop = c["span3"] / c["mfma"], c["loop3"] / c["mfma"]
    print("%s: %d MFMAs, three-input instructions per MFMA: %.3f between first and last MFMA, %.3f in the tile loop (bound %.2f)"
          % (kernel, c["mfma"], per_span, per_loop, bound))
    assert per_span <= bound, (kernel, per_span)
    assert per_loop <= bound, (kernel, per_loop)
    assert per_loop >= 16 * 1.25 / mfma_per_acc - 1e-9, "fewer than 1.25 instructions per key: the count misses the update"
    assert not c["scratch"], "%s: scratch access inside the tile loop:\n%s" % (kernel, "\n".join(c["scratch"][:8]))


def test_fp4_batch_kernel_keeps_three_waves(product_listing):
    """The 512-query FP4 kernel is built for three waves per SIMD: at most 168 VGPRs, and its spills stay outside the loop."""
    for kernel in ("k_knn2_fp4ILi0ELi4ELi64E", "k_knn2_fp4ILi1ELi4ELi64E"):
        _, meta = S.kernel_body(product_listing, kernel)
        assert meta.get("TotalNumVgprs", 999) <= 168 and meta.get("Occupancy") == 3, (kernel, meta)
        in_loop, _outside = S.scratch_accesses(product_listing, kernel)
        assert not in_loop, "%s: scratch access inside a loop:\n%s" % (kernel, "\n".join(in_loop[:8]))


def test_per_distance_build_is_the_old_update():
    """-DARIA_KNN_TOP2_SINGLE=1 (the A side of A/B measurements, tools/build_ab.sh) keeps two v_med3_f32 per key: 16 keys x 2
    column tiles x 2 per accumulator pair, 256 in the tile loop of the 512-query FP4 kernel, 8 per MFMA; the counter above
    must see that form as over the bound."""
    text = _listing(("-DARIA_KNN_TOP2_SINGLE=1",))
    c = _counts(text, "k_knn2_fp4ILi0ELi4ELi64E")
    loop = _loop_instructions(text, "k_knn2_fp4ILi0ELi4ELi64E")
    assert sum(1 for ln in loop if ln.startswith("v_med3_f32")) == 256 and c["mfma"] == 32
    assert c["loop3"] / c["mfma"] == 8.0 and c["span3"] / c["mfma"] > 5.5
    assert not c["scratch"]
