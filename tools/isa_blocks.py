#!/usr/bin/env python3
"""Static instruction counts of a kernel per basic block, from its gfx950 assembly (hipcc -S --cuda-device-only): VALU, SALU, LDS (ds_*),
global memory and barrier instructions between consecutive labels, and the kernel's totals and register use.  The transform pass
k_ntt_pass4_ct has no loops -- its paths (plain / in_tw / br_src first round) are blocks chosen by uniform branches --, so the blocks a
launch runs add up to its instructions per wave per tile (docs/kernels_2.md, round 7).
Usage: python tools/isa_blocks.py <file.s> <mangled kernel name>"""
import re
import sys


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op == "s_barrier":
        return "barrier"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    keys = ("valu", "salu", "lds", "vmem", "barrier", "wait")
    blocks, cur, name = [], dict.fromkeys(keys, 0), "entry"
    for l in lines[start + 1:end + 1]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append((name, cur))
            cur, name = dict.fromkeys(keys, 0), m.group(1)
            continue
        m = re.match(r"^\s+([a-z]\w+)", l)
        if m and classify(m.group(1)) in cur:
            cur[classify(m.group(1))] += 1
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            cur.setdefault("to", []).append(m.group(1) or m.group(2))
    blocks.append((name, cur))
    total = dict.fromkeys(keys, 0)
    for name, c in blocks:
        if any(c[k] for k in keys):
            print("%-12s" % name, " ".join("%s=%-5d" % (k, c[k]) for k in keys), "->", ",".join(c.get("to", [])))
        for k in keys:
            total[k] += c[k]
    print("%-12s" % "all blocks", " ".join("%s=%-5d" % (k, total[k]) for k in keys))
    for l in lines[end:]:
        m = re.match(r"\s+\.set %s\.(num_vgpr|numbered_sgpr|private_seg_size), (\d+)" % re.escape(kernel), l)
        if m:
            print(m.group(1), m.group(2))
        if l.startswith("\t.section") and kernel not in l and ".AMDGPU" not in l:
            break


if __name__ == "__main__":
    main()
