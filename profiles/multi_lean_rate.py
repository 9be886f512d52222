#!/usr/bin/env python3
"""Re-prints profiles/multi_lean_rate.json: accumulate_multi_kernel with the lean group top against the parent commit -- every run of
the headline A/B (bench.py --gpus 1 --steps 20 --warmup 5, sides alternating), the gain rule, the secondary workloads, the kernel
times and the executed instruction counts per wave.  Needs no GPU:   python profiles/multi_lean_rate.py"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    r = json.load(open(os.path.join(HERE, "multi_lean_rate.json")))
    print(r["what"])
    h = r["cfg3_exact"]
    for side in ("parent", "change"):
        print("cfg3 exact %-6s ms_per_step %s   avg_launch_ms %s" % (side, " ".join("%.2f" % v for v in h[side + "_ms_per_step"]),
                                                                    " ".join("%.2f" % v for v in h[side + "_avg_launch_ms"])))
    print("spread parent %.2f, change %.2f; fastest parent - slowest change %.2f ms: %s (ratio of means %.4f)"
          % (h["parent_spread_ms"], h["change_spread_ms"], h["fastest_parent_minus_slowest_change_ms"],
             "a gain" if h["counts_as_gain"] else "NOT a gain", h["ratio_of_means"]))
    for name, v in r.get("variants_same_session", {}).items():
        print("variant %-28s ms_per_step %s" % (name, " ".join("%.2f" % x for x in v["ms_per_step"])))
    for name, v in r.get("other_once_each", {}).items():
        print("%-14s parent %.2f -> change %.2f ms per step (launch %.2f -> %.2f)" % (name, v["parent"]["ms_per_step"], v["change"]["ms_per_step"],
                                                                                     v["parent"]["avg_launch_ms"], v["change"]["avg_launch_ms"]))
    for side, lines in r.get("kernel_trace", {}).items():
        if isinstance(lines, list):
            for line in lines:
                print("kernel trace %-6s %s" % (side, line))
    c = r.get("counters_per_wave")
    if c:
        for k in sorted(c["parent"]):
            print("%-16s per wave: parent %.1f -> change %.1f" % (k, c["parent"][k], c["change"][k]))
    for line in r.get("dump_outputs", []):
        print(line)


if __name__ == "__main__":
    main()
