#!/usr/bin/env python3
"""Instruction counts of the thirteen partial rounds of the Poseidon2 permutation inside a bulk kernel, from its gfx950 assembly
(hipcc -S --cuda-device-only): everything between the two external round groups.  The external groups are found as the innermost loops
that hold the sixteen S-boxes of a round (more than 100 v_mad_i64_i32); a loop between them (the round-wise form, -DZK_P2_ROUNDWISE) is
weighted by its 13 trips, straight-line code (the deferred form) once.  Classes and costs are those of tools/isa_mix.py: multiply-class
4.2 issue cycles per wave64 instruction, other VALU 2.2; scalar instructions are counted (ALU, memory, s_nop, s_waitcnt) and priced
at one issue cycle each in a column of their own -- they issue beside another wave's VALU, so the VALU column is the floor.
Usage: python tools/partial_rounds_mix.py <file.s> <mangled kernel name> [out.json]"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import CYC_FULL, CYC_MUL, MUL_CLASS  # noqa: E402


def region_counts(path, kernel):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start + 1:end]
    label_at = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            loops.append((label_at[m.group(1)], i))
    inner = sorted(lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops))
    ext = [lp for lp in inner if sum("v_mad_i64_i32" in l for l in body[lp[0]:lp[1] + 1]) > 100]
    if len(ext) != 2:
        sys.exit("expected the two external round loops, found %d" % len(ext))
    lo, hi = ext[0][1] + 1, ext[1][0]
    weight = [1] * len(body)
    between = [lp for lp in inner if lo <= lp[0] and lp[1] < hi]
    for a, b in between:
        for i in range(a, b + 1):
            weight[i] = 13
    c = {"valu_multiply_class": 0, "valu_other": 0, "salu": 0, "smem_loads": 0, "s_nop": 0, "s_waitcnt": 0}
    hist = {}
    for i in range(lo, hi):
        m = re.match(r"^\s+([sv]_\w+)", body[i])
        if not m:
            continue
        op = re.sub(r"_e32$|_e64$|_dpp$|_sdwa$", "", m.group(1))
        w = weight[i]
        hist[op] = hist.get(op, 0) + w
        if op.startswith("v_"):
            c["valu_multiply_class" if op.startswith(MUL_CLASS) else "valu_other"] += w
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            c["smem_loads"] += w
        elif op in ("s_nop", "s_waitcnt"):
            c[op] += w
        else:
            c["salu"] += w
    valu_cycles = CYC_MUL * c["valu_multiply_class"] + CYC_FULL * c["valu_other"]
    scalar = c["salu"] + c["smem_loads"] + c["s_nop"] + c["s_waitcnt"]
    return {"kernel": kernel, "form": "round-wise loop x 13" if between else "straight line", "counts": c,
            "valu_instructions": c["valu_multiply_class"] + c["valu_other"], "modelled_valu_issue_cycles": round(valu_cycles, 1),
            "scalar_instructions": scalar, "modelled_cycles_with_scalar_at_1": round(valu_cycles + scalar, 1),
            "code_lines_between_the_external_groups": hi - lo, "top_opcodes": dict(sorted(hist.items(), key=lambda kv: -kv[1])[:12])}


if __name__ == "__main__":
    out = json.dumps(region_counts(sys.argv[1], sys.argv[2]), indent=1)
    print(out)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(out + "\n")
