#!/usr/bin/env python3
"""Static instruction counts of one kernel in a gfx950 assembly listing (hipcc --save-temps).

    python profiles/r07/isa_counts.py LISTING.s SYMBOL_PREFIX [SYMBOL_PREFIX ...]

Prints, per kernel whose mangled name starts with a prefix: lines of code, instructions by class (scalar ALU, branch, wait,
vector ALU, LDS, lane permute, vector memory load / store) and the register and spill counts of its metadata block.  Static
counts: what the kernel holds, not what a wave executes.
"""
import re
import sys


def body(text, sym):
    m = re.search(r"^%s:.*\n" % re.escape(sym), text, flags=re.M)
    end = text.index(".Lfunc_end", m.end())
    return text[m.end():end]


def classify(op):
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_nop", "s_barrier", "s_endpgm", "s_sleep")):
        return "other"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("ds_bpermute", "ds_permute", "ds_swizzle")):
        return "permute"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_load", "flat_load", "buffer_load", "scratch_load")):
        return "vmem_load"
    if op.startswith(("global_store", "flat_store", "buffer_store", "scratch_store")):
        return "vmem_store"
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    return "other"


def meta(text, sym):
    # (the keys of a kernel's metadata entry are sorted: the register counts follow its .name)
    at = re.search(r"\.name:\s+%s\n" % re.escape(sym), text).end()
    out = {}
    for key in ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count"):
        out[key] = re.compile(r"\.%s:\s+(\d+)" % key).search(text, at).group(1)
    return out


def main():
    text = open(sys.argv[1]).read()
    syms = sorted(set(re.findall(r"^(_Z\w+):", text, flags=re.M)))
    for pre in sys.argv[2:]:
        for sym in [s for s in syms if s.startswith(pre)]:
            lines = [ln.strip() for ln in body(text, sym).splitlines()]
            ops = [ln.split()[0] for ln in lines if ln and not ln.startswith((";", ".", "//")) and not ln.endswith(":")]
            counts = {}
            for op in ops:
                k = classify(op)
                counts[k] = counts.get(k, 0) + 1
            print(sym)
            print("  instructions %d  " % len(ops) + "  ".join("%s %d" % kv for kv in sorted(counts.items())))
            print("  " + "  ".join("%s %s" % kv for kv in meta(text, sym).items()))


if __name__ == "__main__":
    main()
