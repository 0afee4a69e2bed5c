#!/usr/bin/env python
"""Per-scene time steps and frame schedules in one SceneBatch (run_frames) against the ways a mixed batch ran before it, on 8 scenes
of 100 k particles at n_grid 50 with the frame lengths of the reference configs: 4 x jelly (dt 1e-4, 400 substeps per frame),
2 x sand (2e-5, 2 000), 2 x snow (1e-5, 1 000).  Every frame exports all particles with covariances, as gs_simulation.py does.

    python scripts/mpm_schedule_bench.py [--frames F] [--out file.json]
    python scripts/mpm_schedule_bench.py --quick          # only (a), for a kernel trace (rocprofv3 --kernel-trace --stats -- ...)

Variants ("mixed" configuration):
  (a) frames   SceneBatch.run_frames: one schedule per scene;
  (b) solo     each scene's frame loop (export_frame_for_rendering, run) one scene after the other;
  (c) streams  the same frame loops, one HIP stream and host thread per scene (what run_batch does);
  (d) groups   the manual workaround: one SceneBatch per dt group, groups one after the other, frame loop of SceneBatch.run + exports.
"equal" configuration (8 x jelly, equal dt and frame length): (a) against (e) scalar, a SceneBatch.run(dt, steps_per_frame) loop plus
the solo exports.
Each variant has its own solvers, warmed up through the first re-binnings; the timed region synchronises the device on both sides;
variants alternate, median of `--reps`.  The launch count of a variant comes from one more, untimed repetition under the torch
profiler (every kernel launch, re-binning kernels included)."""
import argparse
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixie_amd import mpm_solver  # noqa: E402
from pixie_amd.mpm_solver import FrameSchedule, MPM_Simulator_WARP, SceneBatch  # noqa: E402
from pixie_amd.synthetic import apply_scene, mpm_ball_scene, mpm_plastic_scene  # noqa: E402

mpm_solver.VERBOSE = False
N, NG = 100_000, 50
KINDS = {"jelly": (1e-4, 400), "sand": (2e-5, 2000), "snow": (1e-5, 1000)}


def scene(kind, seed):
    if kind == "jelly":
        return mpm_ball_scene(N, seed=seed, n_grid=NG, scenario=("tree", "ball")[seed % 2])
    if kind == "sand":
        sc = mpm_ball_scene(N, seed=seed, n_grid=NG, scenario="sand")
        sc["per_particle"] = False
        return sc
    sc = mpm_plastic_scene("snow", N, seed=seed)
    sc["n_grid"] = NG
    return sc


def solver(sc):
    s = MPM_Simulator_WARP(10)
    s.load_initial_data_from_torch(torch.from_numpy(sc["x"]), torch.from_numpy(sc["vol"]), torch.from_numpy(sc["cov"]),
                                   n_grid=sc["n_grid"], grid_lim=sc["grid_lim"])
    apply_scene(s, sc, per_particle=sc.get("per_particle", True))
    for name, key in (("F_trial", "F0"), ("v", "v0")):
        if key in sc:
            s.set_field(name, torch.from_numpy(np.ascontiguousarray(sc[key].reshape(sc[key].shape[0], -1))))
    return s


def frame_loop(s, q):
    for _ in range(q.n_frames):
        s.export_frame_for_rendering(q.gs_num, q.scale_origin, q.original_mean_pos, q.rotation_matrices, q.z_shift_value, q.with_cov)
        s.run(q.dt, q.steps_per_frame)


def make_variants(kinds, frames, names):
    scheds = [FrameSchedule(KINDS[k][0], KINDS[k][1], frames, gs_num=N, scale_origin=0.5, original_mean_pos=[0.0, 0.0, 0.0])
              for k in kinds]
    scs = [scene(k, 10 + i) for i, k in enumerate(kinds)]
    out = {}
    for v in names:
        sv = [solver(sc) for sc in scs]
        if v == "frames":
            b = SceneBatch(sv)
            out[v] = (sv, [b], lambda b=b: b.run_frames(scheds))
        elif v == "solo":
            out[v] = (sv, [], lambda sv=sv: [frame_loop(s, q) for s, q in zip(sv, scheds)])
        elif v == "streams":
            streams = [torch.cuda.Stream() for _ in sv]

            def run(sv=sv, streams=streams):
                cur = torch.cuda.current_stream()
                dev = torch.cuda.current_device()

                def work(s, q, st):
                    torch.cuda.set_device(dev)
                    with torch.cuda.stream(st):
                        frame_loop(s, q)
                for st in streams:
                    st.wait_stream(cur)
                th = [threading.Thread(target=work, args=a) for a in zip(sv, scheds, streams)]
                for t in th:
                    t.start()
                for t in th:
                    t.join()
                for st in streams:
                    cur.wait_stream(st)
            out[v] = (sv, [], run)
        elif v in ("groups", "scalar"):
            groups = {}
            for s, q in zip(sv, scheds):
                groups.setdefault((q.dt, q.steps_per_frame), []).append((s, q))
            batches = [(SceneBatch([s for s, _ in g]), g) for g in groups.values()]

            def run(batches=batches):
                for b, g in batches:
                    q0 = g[0][1]
                    for _ in range(q0.n_frames):
                        for s, q in g:
                            s.export_frame_for_rendering(q.gs_num, q.scale_origin, q.original_mean_pos, q.rotation_matrices,
                                                         q.z_shift_value, q.with_cov)
                        b.run(q0.dt, q0.steps_per_frame)
            out[v] = (sv, [b for b, _ in batches], run)
    return scheds, out


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(names), sum("grid_block" in n for n in names)


def measure(config, kinds, frames, names, reps, count_launches=True):
    scheds, var = make_variants(kinds, frames, names)
    for v in names:                                   # warm-up: first binning, re-binning cadence settled
        sv, batches, _ = var[v]
        for s, q in zip(sv, scheds):
            s.run(q.dt, 50)
        torch.cuda.synchronize()
    ps = sum(q.steps_per_frame * q.n_frames for q in scheds) * N     # particle-steps of one repetition
    times = {v: [] for v in names}
    for _ in range(reps):
        for v in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            var[v][2]()
            torch.cuda.synchronize()
            times[v].append(time.perf_counter() - t0)
    rows = []
    for v in names:
        t = sorted(times[v])[len(times[v]) // 2]
        n_launch, n_grid = launches(var[v][2]) if count_launches else (None, None)
        finite = all(bool(torch.isfinite(s.get_field("x")).all()) for s in var[v][0])
        rows.append({"config": config, "variant": v, "scenes": len(kinds), "kinds": kinds, "frames": frames,
                     "particle_steps_per_s": ps / t, "ms": 1e3 * t, "reps_ms": [round(1e3 * x, 2) for x in times[v]],
                     "launches": n_launch, "grid_launches": n_grid, "finite": finite})
        print(f"{config:6s} {v:8s} {rows[-1]['particle_steps_per_s']:.3e} particle-steps/s  {rows[-1]['ms']:8.2f} ms  "
              f"reps {rows[-1]['reps_ms']}  launches {n_launch} (grid {n_grid})  finite {finite}", flush=True)
    for v in names:
        for b in var[v][1]:
            b.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    mixed = ["jelly"] * 4 + ["sand"] * 2 + ["snow"] * 2
    if a.quick:
        rows = measure("mixed", mixed, a.frames, ["frames"], 1, count_launches=False)
    else:
        rows = measure("mixed", mixed, a.frames, ["frames", "solo", "streams", "groups"], a.reps)
        rows += measure("equal", ["jelly"] * 8, a.frames, ["frames", "scalar"], a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
