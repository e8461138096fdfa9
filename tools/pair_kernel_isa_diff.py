#!/usr/bin/env python3
"""Holds the documents-table instantiations of pair_loss_kernel in two device assemblies of pairs.hip against each other.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S old/pairs.hip -o old.s      (likewise new.s)
    python tools/pair_kernel_isa_diff.py old.s new.s

The words-table form added a template parameter (MUL), so the mangled names differ: a kernel is identified by its <V, NITER, G, LAZY>
and, in an assembly that has the parameter, MUL = false. Compared per kernel: the instruction stream (labels and symbol names
normalised, comments dropped) and the register / LDS / scratch figures of its metadata. Prints one line per kernel and, with
--words, the figures of the MUL = true instantiations of the second file. Exit status 1 when a kernel differs."""
import re
import sys

NAME = re.compile(r"_ZN6cunvsm\d+_GLOBAL__N_1\d+pair_loss_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])(?:ELb([01]))?EEEvNS_8PairArgsE")


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN6cunvsm\S*pair_loss_kernel\S*):\s*(?:;.*)?$", text, re.M):
        name = m.group(1)
        k = NAME.fullmatch(name)
        if not k:
            continue
        end = text.index(".Lfunc_end", m.end())
        body = []
        for line in text[m.end():end].splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):      # comments, directives and local labels (their numbering is per file)
                if line.startswith(".LBB"):
                    body.append("label")
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r"L\1", line)
            body.append(line.replace(name, "K"))
        meta = {}
        md = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), text, re.S)
        for key in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset"):
            v = re.search(r"\.amdhsa_%s (\S+)" % key, md.group(1)) if md else None
            meta[key] = v.group(1) if v else None
        key = tuple(int(x) for x in k.groups()[:4]) + (int(k.group(5) or 0),)
        out[key] = (body, meta)
    return out


def main():
    words = "--words" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    old, new = kernels(args[0]), kernels(args[1])
    bad = 0
    for key in sorted(k for k in old if k[4] == 0):
        if key not in new:
            print("%s: missing from %s" % (key[:4], args[1])); bad += 1; continue
        same_isa, same_meta = old[key][0] == new[key][0], old[key][1] == new[key][1]
        bad += not (same_isa and same_meta)
        print("<V=%d, NITER=%d, G=%d, LAZY=%d>: %d instructions, vgpr %s sgpr %s lds %s scratch %s: %s" % (
            key[:4] + (len([l for l in new[key][0] if l != "label"]), new[key][1]["next_free_vgpr"], new[key][1]["next_free_sgpr"],
                       new[key][1]["group_segment_fixed_size"], new[key][1]["private_segment_fixed_size"],
                       "identical" if same_isa and same_meta else "DIFFERENT (%s)" % ("instructions" if not same_isa else "metadata"))))
    if words:
        for key in sorted(k for k in new if k[4] == 1):
            b, m = new[key]
            print("words form <V=%d, NITER=%d, G=%d, LAZY=%d>: %d instructions, vgpr %s sgpr %s lds %s scratch %s" % (
                key[:4] + (len([l for l in b if l != "label"]), m["next_free_vgpr"], m["next_free_sgpr"], m["group_segment_fixed_size"],
                           m["private_segment_fixed_size"])))
    print("%d documents-table kernels compared, %d differ" % (len([k for k in old if k[4] == 0]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
