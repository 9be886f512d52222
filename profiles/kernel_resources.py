#!/usr/bin/env python3
"""Register / LDS / spill table of the accumulate kernels, per kernel family and arithmetic contract, and of the outer-misfit
kernels (kiwi_outer.hpp), the misfit-band kernels (kiwi_bands.hpp), the time-scan kernels (kiwi_timescan.hpp), the kernels of the
linear fit's time scan (kiwi_linfit_timescan.hpp), of its candidate evaluation, plain and as the candidate
evaluation's time scan (both kiwi_linfit_candidates_timescan.hpp), with per-receiver shifts (kiwi_linfit_candidates_floating.hpp), of
its joint bootstrap (kiwi_linfit_candidates_bootstrap.hpp; with the shifts kiwi_linfit_candidates_floating_bootstrap.hpp) and
under the amplitude-spectrum norms (kiwi_spectral_candidates.hpp), the time-domain norms (kiwi_waveform_candidates.hpp) and the
floating time-domain norms (kiwi_waveform_candidates_floating.hpp) and the time-domain norms at many origin times
(kiwi_waveform_candidates_timescan.hpp) and their joint bootstrap (kiwi_waveform_candidates_bootstrap.hpp) and the joint bootstrap
under the amplitude-spectrum norms (kiwi_spectral_candidates_bootstrap.hpp) -- the fold kernels that the bootstraps share
(kiwi_candidates_bootstrap.hpp) are listed with each of them --, from the
compiler's own
report (hipcc -Rpass-analysis=kernel-resource-usage; `make -C kiwi_amd/csrc asm FAMILY=n ARITH=exact|fused`).
--text adds the kernels' text sizes in bytes (accumulate families: `make co`, the symbol sizes of the device code object).
Runs on the build machine (no GPU needed):   python profiles/kernel_resources.py [--json out.json] [--text] [--only=multi|bands|timescan|linfit_timescan|linfit_candidates_timescan|linfit_candidates_floating|linfit_candidates_bootstrap|linfit_candidates_floating_bootstrap|spectral_candidates|waveform_candidates|waveform_candidates_floating|waveform_candidates_timescan|waveform_candidates_bootstrap|spectral_candidates_bootstrap]"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kiwi_amd", "csrc")
FAMILIES = {1: "direct", 2: "grouped", 3: "multi", 4: "cell"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", o).replace("void kiwi::", "").replace("void outer::", "outer::").replace("void bands::", "bands::").replace("void timescan::", "timescan::").replace("void linfit_timescan::", "linfit_timescan::").replace("void linfit::", "linfit::").replace("void linfit_candidates_timescan::", "linfit_candidates_timescan::").replace("void linfit_candidates_floating::", "linfit_candidates_floating::").replace("void linfit_candidates_bootstrap::", "linfit_candidates_bootstrap::").replace("void linfit_candidates_floating_bootstrap::", "linfit_candidates_floating_bootstrap::").replace("void candidates_bootstrap::", "candidates_bootstrap::").replace("void spectral_candidates::", "spectral_candidates::").replace("void waveform_candidates::", "waveform_candidates::").replace("void waveform_candidates_floating::", "waveform_candidates_floating::").replace("void waveform_candidates_timescan::", "waveform_candidates_timescan::") for o in out]


KEYS = (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r"\bVGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"),
        ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
        ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def collect_outer():
    """The outer-misfit kernels (kiwi_outer.hpp, namespace outer), compiled into kiwi_hip.o under the exact contract only
    (`make -C kiwi_amd/csrc asm-hip`)."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm-hip"], capture_output=True, text=True)
    rows, cur = [], None
    for line in (r.stderr + r.stdout).split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = None
            for prefix, fam in (("_ZN5outer", "outer"), ("_ZN5bands", "bands"), ("_ZN8timescan", "timescan"),
                                ("_ZN15linfit_timescan", "linfit_timescan"),
                                ("_ZN26linfit_candidates_timescan", "linfit_candidates_timescan"),
                                ("_ZN26linfit_candidates_floating", "linfit_candidates_floating"),
                                ("_ZN27linfit_candidates_bootstrap", "linfit_candidates_bootstrap"),
                                ("_ZN36linfit_candidates_floating_bootstrap", "linfit_candidates_floating_bootstrap"),
                                ("_ZN20candidates_bootstrap", "candidates_bootstrap"),
                                ("_ZN19spectral_candidates", "spectral_candidates"), ("_ZN19waveform_candidates", "waveform_candidates"),
                                ("_ZN28waveform_candidates_floating", "waveform_candidates_floating"),
                                ("_ZN28waveform_candidates_timescan", "waveform_candidates_timescan"),
                                ("_ZN29waveform_candidates_bootstrap", "waveform_candidates_bootstrap"),
                                ("_ZN29spectral_candidates_bootstrap", "spectral_candidates_bootstrap")):
                if m.group(1).startswith(prefix):
                    cur = {"family": fam, "arith": "exact", "mangled": m.group(1)}
                    rows.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in KEYS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return rows


def text_sizes(fam, ar):
    """{mangled kernel name: bytes of text} of one accumulate family and contract"""
    subprocess.run(["make", "-s", "-C", CSRC, "co", "FAMILY=%d" % fam, "ARITH=%s" % ar], capture_output=True, text=True, check=True)
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    out = subprocess.run([readelf, "-s", "-W", os.path.join(CSRC, "build", "accum_%d_%s.co" % (fam, ar))], capture_output=True, text=True, check=True).stdout
    return {f[7]: int(f[2]) for f in (line.split() for line in out.split("\n")) if len(f) == 8 and f[3] == "FUNC"}


def collect(only=None, text=False):
    rows = []
    accum = [f for f, n in FAMILIES.items() if n == only] if only in FAMILIES.values() else ([] if only else FAMILIES)
    for fam in accum:
        for ar in ("exact", "fused"):
            sizes = text_sizes(fam, ar) if text else {}
            r = subprocess.run(["make", "-s", "-C", CSRC, "asm", "FAMILY=%d" % fam, "ARITH=%s" % ar], capture_output=True, text=True)
            txt = r.stderr + r.stdout
            cur = None
            for line in txt.split("\n"):
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    cur = {"family": FAMILIES[fam], "arith": ar, "mangled": m.group(1)}
                    if m.group(1) in sizes:
                        cur["text"] = sizes[m.group(1)]
                    rows.append(cur)
                    continue
                if cur is None:
                    continue
                for key, pat in (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r"\bVGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"),
                                 ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                                 ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
                                 ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
                    m = re.search(pat, line)
                    if m:
                        cur[key] = int(m.group(1))
    if only not in FAMILIES.values():
        shared = "candidates_bootstrap" if only and only.endswith("_bootstrap") else None       # (what every bootstrap launches)
        rows += [r for r in collect_outer() if not only or r["family"] in (only, shared)]
    names = demangle([r["mangled"] for r in rows])
    for r, n in zip(rows, names):
        r["kernel"] = n
        del r["mangled"]
    return rows


def main():
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    text = "--text" in sys.argv
    rows = collect(only[0] if only else None, text)
    print("| kernel | contract | VGPR | AGPR | SGPR | VGPR spills | SGPR spills | scratch B/lane | LDS B | waves/SIMD |%s" % (" text B |" if text else ""))
    print("|---|---|---|---|---|---|---|---|---|---|%s" % ("---|" if text else ""))
    for r in rows:
        print("| `%s` | %s | %d | %d | %d | %d | %d | %d | %d | %d |%s" % (r["kernel"], r["arith"], r.get("vgpr", -1), r.get("agpr", 0), r.get("sgpr", -1),
                                                                         r.get("vgpr_spill", 0), r.get("sgpr_spill", 0), r.get("scratch", 0),
                                                                         r.get("lds", 0), r.get("occupancy", -1), (" %d |" % r.get("text", -1)) if text else ""))
    if "--json" in sys.argv:
        json.dump(rows, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
