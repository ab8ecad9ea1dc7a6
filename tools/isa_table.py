#!/usr/bin/env python3
"""One line a kernel from the ISA the build saves (lib*/obj/isa/*-gfx950.s): VGPRs, SGPRs, LDS bytes, scratch bytes and the
number of instructions, of two builds side by side.  A compile result, not a timing.

    python3 tools/isa_table.py syllable_detector_swift_amd/lib_parent syllable_detector_swift_amd/lib kernels_match kernels_train ...
"""
import os
import re
import sys

KEYS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size"))


def kernels(path):
    """{name: {vgpr, sgpr, lds, scratch, insts}} of one .s file: the counts from its metadata, the instructions counted in the text"""
    text = open(path).read()
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", text.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0])[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(re.search(re.escape(word) + r":\s+(\d+)", block).group(1)) for k, word in KEYS}
    for name in out:
        body = text.split("\n%s:" % name, 1)[1].split("\n.Lfunc_end", 1)[0]
        out[name]["insts"] = sum(1 for line in body.split("\n") if re.match(r"\t[a-z]", line) and not line.startswith("\t."))
    return out


def main():
    parent, this, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    print("# kernel: vgpr sgpr lds scratch insts, parent -> this (a compile result of hipcc --offload-arch=gfx950, not a timing)")
    for f in files:
        tables = [kernels(os.path.join(lib, "obj", "isa", f + "-hip-amdgcn-amd-amdhsa-gfx950.s")) for lib in (parent, this)]
        assert not set(tables[0]) - set(tables[1]), (f, sorted(set(tables[0]) - set(tables[1])))
        for name in tables[1]:
            if name not in tables[0]:                                     # a kernel this build adds
                print("%s %s: %s   <- new" % (f, name, " ".join("%s %d" % (k, tables[1][name][k]) for k in ("vgpr", "sgpr", "lds", "scratch", "insts"))))
        for name in tables[0]:
            a, b = tables[0][name], tables[1][name]
            cols = " ".join("%s %d -> %d" % (k, a[k], b[k]) for k in ("vgpr", "sgpr", "lds", "scratch", "insts"))
            print("%s %s: %s%s" % (f, name, cols, "" if a == b else "   <- differs"))


if __name__ == "__main__":
    main()
