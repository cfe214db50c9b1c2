"""The place-recognition kernels' gfx950 listing (aria_slam_amd/csrc/bow_index.hip, cross-compiled with the Makefile's flags; no
GPU): the compiler's resource metadata says no kernel uses scratch, and the instruction histogram of tools/isa_kernel_stats.py
holds no floating-point atomic. Nothing else is checked here."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_kernel_stats as S   # noqa: E402


@pytest.fixture(scope="module")
def listing():
    csrc = os.path.join(ROOT, "aria_slam_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "bow_index.hip" in re.search(r"^SRC := (.*)$", mk, re.M).group(1).split()
    flags = re.search(r"^FLAGS := (.*?)(?<!\\)$", mk, re.M | re.S).group(1).replace("\\\n", " ").split()
    flags = [f.replace("$(ARCH)", "gfx950").replace("$(ROOT)", ROOT) for f in flags if f != "-shared"]
    out = os.path.join(ROOT, "build", "isa")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "bow_index.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-I" + csrc, "--cuda-device-only", "-S", "-w", "-o", path,
                                                            os.path.join(csrc, "bow_index.hip")])
    return open(path).read()


def test_every_bow_kernel_has_no_scratch_and_no_float_atomics(listing):
    names = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S*k_bow_\S*)", listing, re.M)))
    assert len(names) >= 11, names                                        # ten kernels, the histogram in two forms
    for want in ("counts", "init_words", "hist", "scan", "scatter", "majority", "idf", "store", "score", "topk"):
        assert any(("k_bow_" + want) in n for n in names), (want, names)
    for name in names:
        body, meta = S.kernel_body(listing, name)
        assert len(body) > 5, name
        assert meta.get("ScratchSize", -1) == 0, (name, meta)
        hist, _, _ = S.stats(body)
        assert not any(op.startswith(("global_atomic", "buffer_atomic", "flat_atomic", "ds_")) and ("f32" in op or "f64" in op)
                       and ("add" in op or "min" in op or "max" in op) for op in hist), (name, hist)
