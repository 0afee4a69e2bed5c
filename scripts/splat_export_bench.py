#!/usr/bin/env python
"""Per-frame 3DGS PLY export (gs_simulation.py:290-322 with --save_ply, the reference's default) on one GPU, at 100 k and 350 k
Gaussians (SH degree 3, 62 float columns):

    python scripts/splat_export_bench.py --part kernels              # launches only, for rocprofv3 --kernel-trace --stats -- ...
    python scripts/splat_export_bench.py --part frame [--out f.json] # one PLY frame, split; and the reference's route, restated
    python scripts/splat_export_bench.py --part batch [--out f.json] # SceneBatch.run_frames, 8 x 100 k, with and without splats

"frame", ours: export_frame_splats + the vertex block on the device (kernel), one device-to-host copy (d2h), one file write (write).
"frame", reference route -- restated here from its description, not copied: export_frame_for_rendering (pos, cov), then on the
device torch.linalg.eigh, descending sort, sqrt(clamp(1e-12)), log, det flip of column 2; R to the host and scipy
Rotation.from_matrix(R).as_quat() reordered to wxyz (eigh+scipy); the float64 attribute block filled through list(map(tuple, .))
into the structured array (tuple fill); the file written (write).  Medians of --reps, device synchronised at every split.
"batch": 8 jelly scenes of 100 k particles, 400 substeps of 1e-4 per frame, --frames frames exporting all particles, with_splats on
every scene against off; alternating, median of --reps."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixie_amd import mpm_solver, ply_io, splat_export  # noqa: E402
from pixie_amd.mpm_solver import FrameSchedule, MPM_Simulator_WARP, SceneBatch  # noqa: E402
from pixie_amd.synthetic import apply_scene, mpm_ball_scene  # noqa: E402

mpm_solver.VERBOSE = False
SIZES = (100_000, 350_000)
K = 16      # SH degree 3


def solver(n, seed=0):
    sc = mpm_ball_scene(n, seed=seed, n_grid=50 if n <= 100_000 else 80, scenario="tree")
    s = MPM_Simulator_WARP(10)
    s.load_initial_data_from_torch(torch.from_numpy(sc["x"]), torch.from_numpy(sc["vol"]), torch.from_numpy(sc["cov"]),
                                   n_grid=sc["n_grid"], grid_lim=sc["grid_lim"])
    apply_scene(s, sc)
    s.run(1e-4, 50)                      # a deformed state: F != I
    return s


def frame_args(n):
    c, s_ = np.cos(0.4), np.sin(0.4)
    R = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
    return n, 0.37, torch.tensor([0.1, -0.2, 0.3]), [R]


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def part_kernels(reps):
    for n in SIZES:
        s = solver(n)
        args = frame_args(n)
        for _ in range(reps):
            s.export_frame_for_rendering(*args, z_shift_value=0.05)
            s.export_frame_splats(*args, z_shift_value=0.05)
        torch.cuda.synchronize()
        print(f"{n}: {reps} x frame_export_kernel, {reps} x frame_splat_kernel", flush=True)


def reference_route(s, args, opacity, shs, path):
    from scipy.spatial.transform import Rotation
    t0 = sync_time()
    pos, cov = s.export_frame_for_rendering(*args, z_shift_value=0.05)
    n = cov.shape[0]
    S = cov.new_zeros((n, 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        S[:, a, b] = cov[:, k]
        S[:, b, a] = cov[:, k]
    w, v = torch.linalg.eigh(S)
    idx = torch.argsort(w, dim=1, descending=True)
    w = w.gather(1, idx)
    v = v.gather(2, idx.unsqueeze(1).expand(-1, 3, -1))
    log_s = torch.log(torch.sqrt(torch.clamp(w, min=1e-12)))
    neg = torch.det(v) < 0
    v[neg, :, 2] *= -1
    t1 = sync_time()
    q = Rotation.from_matrix(v.cpu().numpy()).as_quat()[:, [3, 0, 1, 2]]
    t2 = time.perf_counter()
    xyz = pos.cpu().numpy()
    sh = shs[:n].cpu()
    attrs = np.concatenate((xyz, np.zeros_like(xyz), sh[:, :1, :].transpose(1, 2).flatten(1).numpy(),
                            sh[:, 1:, :].transpose(1, 2).flatten(1).numpy(), opacity[:n].cpu().numpy(), log_s.cpu().numpy(), q), axis=1)
    el = np.empty(n, dtype=[(a, "f4") for a in splat_export.attribute_names(K)])
    el[:] = list(map(tuple, attrs))
    t3 = time.perf_counter()
    ply_io.write_ply(path, el)
    t4 = time.perf_counter()
    return {"kernel+eigh": t1 - t0, "scipy": t2 - t1, "tuple_fill": t3 - t2, "write": t4 - t3, "total": t4 - t0}


def ours(s, args, opacity, shs, path):
    t0 = sync_time()
    pos, cov, ls, q = s.export_frame_splats(*args, z_shift_value=0.05)
    block, names = splat_export.vertex_block(pos, ls, q, opacity, shs)
    t1 = sync_time()
    host = block.cpu().numpy()
    t2 = time.perf_counter()
    ply_io.write_ply_f4(path, names, host)
    t3 = time.perf_counter()
    return {"kernel": t1 - t0, "d2h": t2 - t1, "write": t3 - t2, "total": t3 - t0}


def part_frame(reps):
    out = {}
    tmp = tempfile.mkdtemp(prefix="splat_bench_")
    try:
        for n in SIZES:
            s = solver(n)
            args = frame_args(n)
            g = torch.Generator().manual_seed(0)
            opacity = torch.sigmoid(torch.randn((n, 1), generator=g)).cuda()
            shs = torch.randn((n, K, 3), generator=g).cuda()
            rows = {"ours": [], "reference_route": []}
            for r in range(reps + 1):
                a = ours(s, args, opacity, shs, os.path.join(tmp, "ours.ply"))
                b = reference_route(s, args, opacity, shs, os.path.join(tmp, "ref.ply"))
                if r:                                     # the first repetition warms up
                    rows["ours"].append(a)
                    rows["reference_route"].append(b)
            med = {k: {f: float(np.median([x[f] for x in v])) for f in v[0]} for k, v in rows.items()}
            med["file_bytes"] = os.path.getsize(os.path.join(tmp, "ours.ply"))
            out[str(n)] = med
            print(n, json.dumps(med), flush=True)
            del s
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def part_batch(reps, frames):
    n = 100_000
    res = {}
    variants = {}
    for v in ("plain", "splats"):
        sv = [solver(n, seed=20 + i) for i in range(8)]
        scheds = [FrameSchedule(1e-4, 400, frames, gs_num=n, scale_origin=0.37, original_mean_pos=[0.0, 0.0, 0.0],
                                with_splats=(v == "splats")) for _ in sv]
        b = SceneBatch(sv)
        b.run_frames(scheds)                            # warm-up: re-binnings, table allocation
        variants[v] = (sv, b, scheds)
    times = {v: [] for v in variants}
    for _ in range(reps):
        for v, (sv, b, scheds) in variants.items():
            t0 = sync_time()
            b.run_frames(scheds)
            times[v].append(sync_time() - t0)
    for v in variants:
        res[v] = {"median_s": float(np.median(times[v])), "all_s": times[v]}
        print(v, json.dumps(res[v]), flush=True)
    res["splat_overhead_pct"] = 100.0 * (res["splats"]["median_s"] / res["plain"]["median_s"] - 1.0)
    for _, b, _ in variants.values():
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "frame", "batch"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "kernels":
        part_kernels(a.reps)
        return
    res = {"part": a.part, "device": torch.cuda.get_device_name(0)}
    res.update(part_frame(a.reps) if a.part == "frame" else part_batch(a.reps, a.frames))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
