#!/usr/bin/env python
"""Fused multi-scene MPM step (SceneBatch: one launch pair per substep for S scenes) against run_batch (one HIP stream and host thread
per scene) and S solo runs one after the other, on seeded mpm_ball_scene's.

    python scripts/mpm_batch_bench.py [--out file.json] [--quick]
    python scripts/mpm_batch_bench.py --check-trace results.db [--stats-out stats.csv]

Per configuration the three variants have their own solvers, are warmed up through the first re-binning intervals (as bench.py's
bench_mpm_multi_scene), then timed in turn -- fused, streams, solo, fused, ... -- three repetitions each; the median is reported as
particle-steps/s and us per scene-substep, with the re-binnings the timed repetitions went through (each one synchronises the stream).
Variants: "fused" (SceneBatch; every scene keeps its own block-kernel variant, so 100 k scenes -- ~500 work items each, at most 3 per CU --
run the latency-optimised "wide" kernel in the batch too), "fused5" (SceneBatch over scenes with set_scalar("wide", 0): the five-waves-per-SIMD
kernel the 1 M scene runs), "streams" (run_batch), "solo" (the scenes one after the other).
--quick: only the fused 8 x 100 k configuration, for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/mpm_batch_bench.py
--quick); --check-trace then summarises that trace and fails unless the batched kernels ran and the solo block / grid kernels did not."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pixie_amd import mpm_solver  # noqa: E402
from pixie_amd.mpm_solver import MPM_Simulator_WARP, SceneBatch, run_batch  # noqa: E402
from pixie_amd.synthetic import apply_scene, mpm_ball_scene  # noqa: E402

mpm_solver.VERBOSE = False


def solver(sc, wide=None):
    s = MPM_Simulator_WARP(10)
    s.load_initial_data_from_torch(torch.from_numpy(sc["x"]), torch.from_numpy(sc["vol"]), torch.from_numpy(sc["cov"]),
                                   n_grid=sc["n_grid"], grid_lim=sc["grid_lim"])
    apply_scene(s, sc)
    if wide is not None:
        s._set_scalar("wide", wide)
    return s


def rebins(solvers):
    return sum(int(s._get_scalar("n_rebins")) for s in solvers)


def measure(particles, n_grid, s_list, substeps, variants=("fused", "fused5", "streams", "solo"), reps=3):
    pool = max(s_list)
    scenes = [mpm_ball_scene(particles, seed=10 + i, n_grid=n_grid) for i in range(pool)]
    dt = scenes[0]["dt"]
    solvers = {v: [solver(sc, wide=0 if v == "fused5" else None) for sc in scenes] for v in variants}
    rows = []
    for S in s_list:
        sets = {v: solvers[v][:S] for v in variants}
        batches = {v: SceneBatch(sets[v]) for v in variants if v.startswith("fused")}

        def run(v, n):
            if v in batches:
                batches[v].run(dt, n)
            elif v == "streams":
                run_batch(sets[v], dt, n)
            else:
                for s in sets[v]:
                    s.run(dt, n)
            torch.cuda.synchronize()

        for v in variants:
            run(v, 50)
        times = {v: [] for v in variants}
        r0 = {v: rebins(sets[v]) for v in variants}
        for _ in range(reps):
            for v in variants:
                t0 = time.perf_counter()
                run(v, substeps)
                times[v].append(time.perf_counter() - t0)
        n_rebins = {v: rebins(sets[v]) - r0[v] for v in variants}
        for v in variants:
            t = sorted(times[v])[len(times[v]) // 2]
            finite = all(bool(torch.isfinite(s.get_field("x")).all()) for s in sets[v])
            rows.append({"particles": particles, "n_grid": n_grid, "scenes": S, "variant": v, "substeps": substeps,
                         "particle_steps_per_s": S * particles * substeps / t, "us_per_scene_substep": 1e6 * t / (S * substeps),
                         "us_per_substep": 1e6 * t / substeps, "reps_us_per_substep": [round(1e6 * x / substeps, 2) for x in times[v]],
                         "rebins_in_timed_reps": n_rebins[v], "finite": finite})
            print(f"{S:2d} x {particles:>7d} (n_grid {n_grid}) {v:8s} {rows[-1]['particle_steps_per_s']:.3e} particle-steps/s  "
                  f"{rows[-1]['us_per_scene_substep']:7.2f} us per scene-substep  reps {rows[-1]['reps_us_per_substep']}  "
                  f"re-binnings {n_rebins[v]}  finite {finite}", flush=True)
        for b in batches.values():
            b.close()
    return rows


def check_trace(db, stats_out=None):
    """per-kernel calls / mean us of a rocprofv3 trace of --quick; raises unless the launches were the batched kernels"""
    import csv
    import sqlite3
    con = sqlite3.connect(db)
    rows = list(con.execute("select name, total_calls, total_duration, average from top_kernels"))
    if stats_out:
        with open(stats_out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["kernel", "calls", "total_us", "avg_us"])
            for name, calls, tot, avg in rows:
                w.writerow([name[:160], calls, f"{tot:.1f}", f"{avg:.3f}"])
    calls = {}
    for name, c, _, _ in rows:
        calls[name] = calls.get(name, 0) + c
    batched = sum(c for n, c in calls.items() if "mpm_block_batch_kernel" in n or "mpm_grid_block_batch_kernel" in n)
    solo = sum(c for n, c in calls.items() if ("mpm_block_kernel<" in n or "mpm_grid_block_kernel<" in n))
    for name, c, tot, avg in rows[:8]:
        print(f"{c:6d} x {avg:9.3f} us  {name[:110]}")
    print(f"batched kernel launches {batched}, solo block / grid kernel launches {solo}")
    if batched == 0 or solo != 0:
        raise SystemExit("the trace does not show the batched kernels as the hot path")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--check-trace", metavar="DB", default=None)
    ap.add_argument("--stats-out", default=None)
    a = ap.parse_args()
    if a.check_trace:
        check_trace(a.check_trace, a.stats_out)
        return
    if a.quick:
        rows = measure(100_000, 50, [8], 200, variants=("fused",), reps=1)
    else:
        rows = measure(100_000, 50, [1, 2, 3, 4, 8, 16], 200) + measure(1_000_000, 120, [2], 100)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
