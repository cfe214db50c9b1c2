#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two `hipcc -S` device listings of the same source, for changes that must leave the
kernels as they are: instruction count, opcode histogram and the resource metadata of every kernel, one line per kernel.

Usage: isa_compare.py <before.s> <after.s> [more pairs ...]   (exit status 1 when any kernel differs)
The listings come from the Makefile's flags with --cuda-device-only -S, as the _listing() helpers of tests/test_*_host.py
produce them."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_kernel_stats as S   # noqa: E402

META = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(text):
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)


def compare(before, after):
    """[(kernel, instructions before, after, same histogram, same metadata, same text, metadata)] for every kernel of either."""
    a, b = open(before).read(), open(after).read()
    names = kernels(a)
    rows = []
    for k in names + [k for k in kernels(b) if k not in names]:
        if k not in kernels(a) or k not in kernels(b):
            rows.append((k, -1, -1, False, False, False, {}))
            continue
        (ba, ma), (bb, mb) = S.kernel_body(a, k), S.kernel_body(b, k)
        for meta, text in ((ma, a), (mb, b)):      # newer compilers print the scalar registers as TotalNumSgprs
            tail = text[text.index(k + ":"):]
            meta["NumSgprs"] = int(re.search(r"; (?:Total)?NumSgprs: (\d+)", tail).group(1))
        ma, mb = {m: ma.get(m) for m in META}, {m: mb.get(m) for m in META}
        rows.append((k, len(ba), len(bb), S.stats(ba)[0] == S.stats(bb)[0], ma == mb, ba == bb, mb))
    return rows


if __name__ == "__main__":
    bad = 0
    print("listing kernel instructions_before instructions_after histogram metadata text " + " ".join(META))
    for before, after in zip(sys.argv[1::2], sys.argv[2::2]):
        for k, na, nb, hist, meta, text, m in compare(before, after):
            same = na == nb and hist and meta
            bad += not same
            print("%s %s %d %d %s %s %s %s" % (os.path.basename(after), k, na, nb, "equal" if hist else "DIFFERENT",
                                               "equal" if meta else "DIFFERENT", "identical" if text else "reordered",
                                               " ".join(str(m.get(x)) for x in META)))
    sys.exit(1 if bad else 0)
