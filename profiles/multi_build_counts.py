#!/usr/bin/env python3
"""Static instruction counts of accumulate_multi_kernel's build phase, from the compiler's assembly (`make -C kiwi_amd/csrc asm FAMILY=3
ARITH=exact|fused`): for the flagship instantiation <10, true, 4, true, true> and for <10, true, 2, true, true>, the text between the
kernel's priority raise (`s_setprio 1`, in front of the build) and its priority drop (`s_setprio 0`, behind the barrier that ends the
build), cut at every `s_barrier`, every segment counted by instruction class.  The classes go by mnemonic family alone:

  packed      v_pk_*                                   other_vector  every other v_*
  lane        v_readlane / v_readfirstlane / v_writelane
  scalar_alu  every s_* not named below               scalar_load   s_load_* / s_buffer_load_*
  vector_load buffer_* / global_* / flat_* / scratch_*  lds          ds_*
  wait        s_waitcnt* / s_nop / s_sleep            branch        s_branch / s_cbranch_* / s_setpc / s_swappc / s_call
  barrier     s_barrier

This is TEXT, not executed counts: a segment holds every path the compiler laid out between two barriers (the fast and the clamped
row form, the shared and the one-by-one build), in the order of the listing.  `spilled_sgprs` is the compiler's own count of scalar
registers it parks in vector lanes (-Rpass-analysis=kernel-resource-usage).  Runs on the build machine (no GPU needed):

    python profiles/multi_build_counts.py [--json out.json]"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kiwi_amd", "csrc")
KERNELS = ("accumulate_multi_kernel<10, true, 4, true, true>", "accumulate_multi_kernel<10, true, 2, true, true>")
CLASSES = ("packed", "other_vector", "lane", "scalar_alu", "scalar_load", "vector_load", "lds", "wait", "branch", "barrier")


def classify(mn):
    if mn == "s_barrier":
        return "barrier"
    if mn.startswith("v_pk_"):
        return "packed"
    if mn.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return "lane"
    if mn.startswith("v_"):
        return "other_vector"
    if mn.startswith(("s_load_", "s_buffer_load_")):
        return "scalar_load"
    if mn.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if mn.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if mn.startswith("s_"):
        return "scalar_alu"
    if mn.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vector_load"
    if mn.startswith("ds_"):
        return "lds"
    return None


def mangled_name(kernel, arith):
    m = re.match(r"accumulate_multi_kernel<(\d+), (true|false), (\d+), (true|false), (true|false)>", kernel)
    b = lambda s: "Lb1E" if s == "true" else "Lb0E"
    return "_ZN4kiwi5%s23accumulate_multi_kernelILi%sE%sLi%sE%s%sEEv" % (arith, m.group(1), b(m.group(2)), m.group(3), b(m.group(4)), b(m.group(5)))


def instructions(lines):
    """mnemonics of the listing's instruction lines (labels, directives and comments skipped; the lines of an inline assembly statement
    are instructions like the others)"""
    out = []
    for line in lines:
        s = line.split(";", 1)[0].strip()
        if not s or s.startswith((".", "#", "//")) or s.endswith(":"):
            continue
        mn = s.split()[0]
        if classify(mn) is not None:
            out.append(mn)
    return out


def kernel_counts(text, report, kernel, arith):
    name = mangled_name(kernel, arith)
    lines = text.split("\n")
    beg = next(i for i, l in enumerate(lines) if l.startswith(name) and l.split()[0].endswith(":"))
    end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ins = instructions(lines[beg + 1:end])
    sp = [(i, m) for i, m in enumerate(ins) if m == "s_setprio"]
    body = lines[beg + 1:end]
    # the s_setprio lines with their operands, in listing order
    prio = [l.split(";", 1)[0].split()[1] for l in body if l.split(";", 1)[0].strip().startswith("s_setprio")]
    assert len(prio) == len(sp)
    first = next(i for (i, _), p in zip(sp, prio) if p == "1")
    last = max(i for (i, _), p in zip(sp, prio) if p == "0")
    assert first < last, "priority raise behind the drop"
    segs, cur = [], dict.fromkeys(CLASSES, 0)
    for mn in ins[first + 1:last]:
        c = classify(mn)
        if c == "barrier":
            cur["barrier"] = 1
            segs.append(cur)
            cur = dict.fromkeys(CLASSES, 0)
            continue
        if mn != "s_setprio":
            cur[c] += 1
    segs.append(cur)
    for s in segs:
        s["all"] = sum(s[c] for c in CLASSES)
    total = {c: sum(s[c] for s in segs) for c in CLASSES + ("all",)}
    whole = dict.fromkeys(CLASSES, 0)
    for mn in ins:
        whole[classify(mn)] += 1
    whole["all"] = len(ins)
    sym = lines[beg].split()[0].rstrip(":")
    m = re.search(r"Function Name: %s\b.*\n(?:.*\n){0,16}?.*SGPRs Spill: (\d+)" % re.escape(sym), report)
    return {"kernel": kernel, "arith": arith, "raise_to_drop": {"segments": segs, "total": total}, "whole_kernel": whole,
            "priority_raises": prio.count("1"), "priority_drops": prio.count("0"), "spilled_sgprs": int(m.group(1)) if m else -1}


def collect():
    rows = []
    for ar in ("exact", "fused"):
        r = subprocess.run(["make", "-s", "-C", CSRC, "asm", "FAMILY=3", "ARITH=%s" % ar, "PYTHON=" + sys.executable], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("make asm failed:\n" + r.stderr[-2000:])
        text = open(os.path.join(CSRC, "build", "accum_3_%s.s" % ar)).read()
        for k in KERNELS:
            rows.append(kernel_counts(text, r.stderr + r.stdout, k, ar))
    return rows


def main():
    rows = collect()
    for r in rows:
        print("%s  %s  (scalars parked in vector lanes: %d)" % (r["kernel"], r["arith"], r["spilled_sgprs"]))
        print("  segment      " + " ".join("%12s" % c for c in CLASSES + ("all",)))
        for i, s in enumerate(r["raise_to_drop"]["segments"]):
            print("  %-12d " % i + " ".join("%12d" % s[c] for c in CLASSES + ("all",)))
        print("  raise-drop   " + " ".join("%12d" % r["raise_to_drop"]["total"][c] for c in CLASSES + ("all",)))
        print("  whole kernel " + " ".join("%12d" % r["whole_kernel"][c] for c in CLASSES + ("all",)))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
