"""`bench.py`'s default line, a built checkout of the parent commit and this build alternating in one session, two runs each: what
the plain path costs before and after a change that does not touch it.  Writes profiles/waveform_candidates_time_scan_default_line.json.

    git worktree add --detach <dir> <parent commit>;  (cd <dir> && python -c "import __graft_entry__ as g; g.build()")
    python profiles/waveform_candidates_time_scan_default_line.py --parent=<dir> [out.json] [--label=<parent commit>] [--steps=30] [--warmup=5]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    parent = os.path.abspath(opt["parent"])
    steps, warmup = int(opt.get("steps", 30)), int(opt.get("warmup", 5))
    label = "parent " + opt.get("label", os.path.basename(parent))
    runs = []
    for order, (name, cwd) in enumerate([(label, parent), ("this build", ROOT)] * 2, 1):
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=cwd,
                             capture_output=True, text=True, timeout=280)
        if out.returncode != 0:
            sys.exit("%s: bench.py failed\n%s" % (name, out.stderr[-2000:]))
        r = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
        runs.append(dict(order=order, build=name, ms_per_step=r["ms_per_step"], evals_per_s=r["value"], steps=steps, warmup=warmup))
        print(json.dumps(runs[-1]), flush=True)
    import torch
    P = [r["ms_per_step"] for r in runs if r["build"] == label]
    T = [r["ms_per_step"] for r in runs if r["build"] == "this build"]
    res = dict(what="bench.py --gpus 1 --steps %d --warmup %d (the default line), a checkout of the parent commit and this build alternating "
                    "in one session, two runs each" % (steps, warmup),
               device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), runs=runs,
               parent_mean_ms_per_step=sum(P) / len(P), this_mean_ms_per_step=sum(T) / len(T), parent_spread_ms=max(P) - min(P),
               this_spread_ms=max(T) - min(T), this_over_parent=sum(T) / sum(P),
               pairs_overlap=bool(min(T) <= max(P) and min(P) <= max(T)),
               note="the plain path's code is not touched by this change; the margin is the spread between the parent's own runs")
    print(json.dumps(res))
    with open(args[0] if args else os.path.join(ROOT, "profiles", "waveform_candidates_time_scan_default_line.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
