"""The bootstrap of a grid search on the device: MisfitGrid.postprocess(bootstrap_iterations=1000, engine=...) over the
10^5-point grid of configuration 5's size (100 000 sources x 50 receivers x 3 components, random misfits and norms), both
outer norms -- upload, kernels and download of the one kiwi_hip_outer_misfits call by HIP events, the whole postprocess by
the host clock -- against the host path (postprocess without an engine: 5 draws timed, scaled to 1000) on the same box,
and against the evaluation of the same 10^5 sources (`bench.py --gpus 1 --workload cfg5 --sweep 100000`, a child process
of its own, run first).  The aim: the device postprocess takes less than the sweep.

    python profiles/bootstrap_rate.py [out.json] [--commit=<id>] [--sweep-s=<seconds>: take this instead of running bench.py]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS, NREC, NK, NDRAW, HOST_DRAWS = 100000, 50, 3, 1000, 5


def sweep_seconds():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg5", "--sweep", str(NS)],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    if out.returncode != 0:
        raise RuntimeError("bench.py --sweep failed:\n" + out.stdout[-2000:] + out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    return float(res["wall_s"]), res


def random_grid(seed=1):
    from kiwi_amd import gridsearch, synthetic
    rng = np.random.default_rng(seed)
    base = np.array(synthetic.TRUE_BILAT, np.float32)
    grid = gridsearch.MisfitGrid("bilateral", base, param_values=[("strike", np.linspace(0.0, 359.0, 100)),
                                                                  ("dip", np.linspace(1.0, 90.0, 100)),
                                                                  ("slip-rake", np.linspace(-180.0, 170.0, 10))])
    assert len(grid.sources) == NS
    scale = 10.0 ** rng.uniform(-2, 2, (1, NREC, 1))
    nor = np.repeat((scale * rng.uniform(0.5, 1.5, (1, NREC, NK))).astype(np.float32).astype(np.float64), NS, 0)
    mis = (nor * rng.uniform(0.1, 2.0, (NS, NREC, NK))).astype(np.float32).astype(np.float64)
    grid.misfits_by_src, grid.norms_by_src, grid.failings = mis, nor, []
    grid.ref_misfits_by_src, grid.ref_norms_by_src = mis[:1], nor[:1]
    grid.receiver_mask, grid.nreceivers, grid.ncomponents = np.ones(NREC, bool), NREC, [NK] * NREC
    return grid


def timed(f):
    t = time.perf_counter()
    f()
    return time.perf_counter() - t


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    res = dict(case="%d sources x %d receivers x %d components, %d draws" % (NS, NREC, NK, NDRAW))
    if "sweep-s" in opt:
        res["sweep_s"], res["sweep_source"] = float(opt["sweep-s"]), "given on the command line"
    else:
        res["sweep_s"], line = sweep_seconds()
        res["sweep_source"] = "bench.py --gpus 1 --workload cfg5 --sweep %d, same session" % NS
        res["sweep_evals_per_s"] = line["value"]
    print("sweep of %d sources: %.2f s" % (NS, res["sweep_s"]), flush=True)
    import torch
    from kiwi_amd import Engine
    res["device"] = "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName)
    grid = random_grid()
    e = Engine(0)
    e.outer_misfits(grid.misfits_by_src[:512], grid.norms_by_src[:512], ncomponents=grid.ncomponents)      # code objects, buffers
    for outer_norm in ("l2norm", "l1norm"):
        r = {}
        whole = [timed(lambda: grid.postprocess(NDRAW, np.random.default_rng(5), engine=e, outer_norm=outer_norm)) for _ in range(3)]
        up, kern, down = e.outer_ms()
        draws = np.concatenate([np.ones((1, NREC)), np.ones((NDRAW, NREC))], 0)
        call = [timed(lambda: e.outer_misfits(grid.misfits_by_src, grid.norms_by_src, outer_norm, draw_weights=draws, which_draw=0,
                                              ncomponents=grid.ncomponents)) for _ in range(3)]
        dev_best, dev_boot = grid.ibest, np.array(grid.bootstrap_sources[:HOST_DRAWS])
        r["device"] = dict(postprocess_s=float(np.median(whole)), postprocess_s_runs=whole, upload_ms=up, kernels_ms=kern, download_ms=down,
                           outer_misfits_call_s=float(np.median(call)),      # host clock: float32 copies of the arrays + the C-ABI call
                           fp64_ops=4.0 * NS * NREC * (NDRAW + 1), kernel_tflops=4.0 * NS * NREC * (NDRAW + 1) / (kern * 1e-3) / 1e12)
        t0 = timed(lambda: grid.postprocess(0, np.random.default_rng(5), outer_norm=outer_norm))
        t5 = timed(lambda: grid.postprocess(HOST_DRAWS, np.random.default_rng(5), outer_norm=outer_norm))
        per_draw = (t5 - t0) / HOST_DRAWS
        r["host"] = dict(without_draws_s=t0, s_per_draw=per_draw, draws_timed=HOST_DRAWS, scaled_to_1000_draws_s=t0 + NDRAW * per_draw)
        r["same_best_source"] = bool(grid.ibest == dev_best)
        r["same_first_bootstrap_sources"] = bool(np.array_equal(np.array(grid.bootstrap_sources), dev_boot))
        r["host_over_device"] = r["host"]["scaled_to_1000_draws_s"] / r["device"]["postprocess_s"]
        r["device_postprocess_over_sweep"] = r["device"]["postprocess_s"] / res["sweep_s"]
        res[outer_norm] = r
        print(outer_norm, json.dumps(r), flush=True)
    res["aim_met"] = bool(all(res[n]["device_postprocess_over_sweep"] < 1.0 for n in ("l2norm", "l1norm")))
    e.close()
    res["commit"] = opt.get("commit")
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                                    stderr=subprocess.DEVNULL).strip()
        except Exception:
            pass
    print(json.dumps(res))
    if args:
        with open(args[0], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
