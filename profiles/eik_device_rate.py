"""What the device march (kiwi_amd/csrc/kiwi_fmm_device.hpp, one fast-marching solve per wavefront) delivers, written to
profiles/eik_device_rate.json.  Usage: python profiles/eik_device_rate.py [--quick] [--out FILE]

1. cfg4's 1200 x 360 grid of 25 m (the field of tests/test_fast_marching.py::test_cfg4_sized_grid_against_the_plain_routine,
   another start point per solve): device solves per second, kernel ms, ns per node the march has to accept and the heap's
   high-water mark for 128, 512, 1024 and 2048 solves per call; the host's solves per second on 1, 2 and 16 threads.
2. End to end: 512 cfg4-nukl trials (the list bench.py --workload cfg4-nukl uses) through Engine.make_misfits_for_sources, host
   solver against device solver, each with KIWI_HIP_DISC_THREADS 2 and 16, each in a fresh child process with the per-piece
   trace on; misfits compared bit for bit between the four runs.
Median of the repeats after a warm-up call; the spread (min, max) is kept."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                             # noqa: E402

KERNEL = {"name": "fmm_batch_kernel", "vgprs": 35, "sgprs": 94, "scratch_bytes": 0, "lds_bytes_per_workgroup": 32768,
          "workgroup": 64, "waves_per_cu": 5, "source": "make -C kiwi_amd/csrc asm-hip (gfx950); waves per CU = 160 KB of LDS / 32 KB"}


def cfg4_problem(n):
    from tests.test_fmm_batch import cfg4_field, cfg4_starts
    speed, origin, delta, dis = cfg4_field()
    return speed, origin, delta, dis, cfg4_starts(n, seed=11)


def raw_batch(L, h, where, speed, origin, delta, dis, starts):
    """n solves over the same field through the C-ABI (no per-solve Python arrays: 2048 solves are 3.5 GB of speeds)."""
    n = len(starts)
    nn = speed.size
    nx = np.full(n, speed.shape[1], np.int32)
    ny = np.full(n, speed.shape[0], np.int32)
    ofs = (np.arange(n, dtype=np.int64) * nn)
    packed = np.tile(speed.ravel(), n)
    times = np.zeros(n * nn, np.float32)
    org = np.tile(origin, (n, 1)).astype(np.float32)
    dlt = np.tile(delta, (n, 1)).astype(np.float32)
    sta = np.ascontiguousarray(starts, np.float32)
    dd = np.full(n, dis, np.float32)
    fb = C.c_longlong(0)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))        # noqa: E731

    def call():
        t0 = time.perf_counter()
        rc = L.kiwi_hip_fast_marching_batch(h, where, n, ip(nx), ip(ny), ofs.ctypes.data_as(C.POINTER(C.c_longlong)), fp(packed), fp(org),
                                            fp(dlt), fp(sta), fp(dd), fp(times), C.byref(fb))
        assert rc == 0
        return time.perf_counter() - t0, fb.value
    return call, times


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def child(solver, out):
    import bench
    from kiwi_amd import synthetic
    wl = synthetic.workload("cfg4-nukl", 512)
    p = bench.setup_product(0, wl, 4096)[0]
    p.set_eikonal_solver(solver)
    tr = wl["trials"]
    p.make_misfits_for_sources(wl["sourcetype"], tr[:128])      # warm-up: code objects, buffers, thread team
    rates = []
    for rep in range(3):
        p.L.kiwi_hip_eikonal_cache_stats(None, None, 3)
        sys.stderr.write("== repeat %d\n" % rep)
        t0 = time.perf_counter()
        mis, nor, failings = p.make_misfits_for_sources(wl["sourcetype"], tr)
        rates.append(len(tr) / (time.perf_counter() - t0))
    np.save(out, np.concatenate([mis.ravel(), nor.ravel()]))
    print(json.dumps({"evals_per_s": spread(rates), "failings": len(failings), "eikonal_solver_ms": p.eikonal_solver_ms(),
                      "eikonal_solver_stats": p.eikonal_solver_stats()}))


def main():
    quick = "--quick" in sys.argv
    from kiwi_amd import Engine, lib as klib
    L = klib.load()
    res = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or os.environ.get("KIWI_COMMIT", "unknown"),
           "cpu": next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "?"),
           "effective_cpus": L.kiwi_hip_effective_cpus(), "kernel": KERNEL, "grid": "1200 x 360 nodes of 25 m, early termination (discard)"}
    eng = Engine(0)
    sizes = [128, 512] if quick else [128, 512, 1024, 2048]
    speed, origin, delta, dis, starts = cfg4_problem(max(sizes))
    kept = int((speed != np.float32(dis)).sum())
    call, _ = raw_batch(L, eng.h, 1, speed, origin, delta, dis, starts[:128])
    call()                                                        # warm-up
    dev = {}
    for n in sizes:
        call, times = raw_batch(L, eng.h, 1, speed, origin, delta, dis, starts[:n])
        wall, kern, fbs = [], [], 0
        for rep in range(3 if n <= 512 else 2):
            dt, fb = call()
            up, k, down = eng.eikonal_solver_ms()
            wall.append(n / dt); kern.append(k); fbs += fb
        launches, hiwater = eng.eikonal_solver_stats()
        kmed = spread(kern)["median"]
        dev[str(n)] = {"solves_per_s_wall": spread(wall), "solves_per_s_kernel": n / (kmed * 1e-3), "kernel_ms": spread(kern),
                       "upload_ms": up, "download_ms": down, "launches": launches, "heap_high_water": hiwater, "fallbacks": fbs,
                       "ns_per_kept_node_per_solve_slot": kmed * 1e6 / kept / max(1.0, n / 1280.0),
                       "ns_per_kept_node_throughput": kmed * 1e6 / (kept * n)}
        print("device, %4d solves per call: %s" % (n, json.dumps(dev[str(n)])), flush=True)
        if n == 128:                                              # the device's times against the host's, bit for bit
            hcall, htimes = raw_batch(L, None, 0, speed, origin, delta, dis, starts[:n])
            hcall()
            dev[str(n)]["bit_identical_to_host"] = bool(np.array_equal(times.view(np.uint32), htimes.view(np.uint32)))
            assert dev[str(n)]["bit_identical_to_host"]
        del times
    res["device"] = dev
    res["kept_nodes_per_solve"] = kept
    host = {}
    for th in (1, 2, 16):
        os.environ["KIWI_HIP_DISC_THREADS"] = str(th)
        n = 16 * th if th < 16 else 128
        call, _ = raw_batch(L, None, 0, speed, origin, delta, dis, starts[:n])
        call()
        r = []
        for rep in range(3):
            dt, fb = call()
            r.append(n / dt)
        host[str(th)] = {"solves_per_s": spread(r), "solves_per_call": n}
        print("host, %2d threads: %s" % (th, json.dumps(host[str(th)])), flush=True)
    os.environ.pop("KIWI_HIP_DISC_THREADS")
    res["host"] = host
    eng.close()
    if not quick:
        e2e, outs = {}, {}
        import tempfile
        tmp = tempfile.mkdtemp()
        for solver in ("host", "device"):
            for th in (2, 16):
                key = "%s_%d_threads" % (solver, th)
                out = os.path.join(tmp, "eik_e2e_%s.npy" % key)
                env = dict(os.environ, KIWI_HIP_DISC_THREADS=str(th), KIWI_HIP_TRACE_PIECES="1")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", solver, out], capture_output=True, text=True, env=env, timeout=900)
                assert r.returncode == 0, r.stderr[-3000:]
                e2e[key] = json.loads(r.stdout.strip().splitlines()[-1])
                e2e[key]["piece_trace_last_repeat"] = [l for l in r.stderr.split("== repeat 2\n")[-1].splitlines() if l.startswith("kiwi_hip piece")]
                outs[key] = np.load(out)
                os.remove(out)
                print("end to end, %s: %s" % (key, json.dumps(e2e[key]["evals_per_s"])), flush=True)
        first = outs["host_2_threads"]
        e2e["misfits_bit_identical_between_the_four_runs"] = bool(all(first.tobytes() == o.tobytes() for o in outs.values()))
        for th in (2, 16):
            e2e["device_over_host_at_%d_threads" % th] = e2e["device_%d_threads" % th]["evals_per_s"]["median"] / e2e["host_%d_threads" % th]["evals_per_s"]["median"]
        res["end_to_end_512_cfg4_nukl"] = e2e
    dst = os.path.join(ROOT, "profiles", "eik_device_rate_quick.json" if quick else "eik_device_rate.json")
    if "--out" in sys.argv:
        dst = sys.argv[sys.argv.index("--out") + 1]
    json.dump(res, open(dst, "w"), indent=1)
    print("written", dst)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
