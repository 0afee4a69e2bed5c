#!/usr/bin/env python
"""Times pixie_amd.scene_ingest.ingest_scene -- from the uploaded PLY block to the outputs ready on the device -- against the same
span (gs_simulation.py:403-438) written as the reference's torch expressions on the same device, at 100 k and 350 k Gaussians, SH
degree 3, two rotations and a sim_area.  Warm-up, then the median of `--reps` calls, each ended by a device synchronise and timed
with the host clock; the two routes alternate.  Recorded, not asserted: writes a table (default profiles/scene_ingest_table.txt).

    python scripts/bench_scene_ingest.py [--sizes 100000 350000] [--reps 30] [--warmup 5] [--out PATH]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pixie_amd.scene_ingest import GaussianCheckpoint, generate_rotation_matrices, ingest_scene  # noqa: E402
from pixie_amd.splat_export import attribute_names  # noqa: E402

CFG = dict(opacity_threshold=0.3, rotation_degree=[30.0, -75.0], rotation_axis=[0, 2], sim_area=[-0.8, 0.75, -0.85, 0.7, -0.75, 0.8],
           z_shift_value=0.3)


def checkpoint(n, k, seed):
    rng = np.random.default_rng(seed)
    names = attribute_names(k)
    block = rng.normal(0, 0.5, (n, len(names))).astype(np.float32)
    col = {nm: i for i, nm in enumerate(names)}
    block[:, [col["x"], col["y"], col["z"]]] = rng.uniform(-1, 1, (n, 3))
    block[:, col["opacity"]] = rng.normal(0, 2, n)
    block[:, [col["scale_0"], col["scale_1"], col["scale_2"]]] = rng.normal(-4, 0.7, (n, 3))
    return GaussianCheckpoint(block, names, int(round(k ** 0.5)) - 1)


def torch_span(ck, cfg, rots):
    """the reference's expressions (GaussianModel accessors, load_params_from_gs, :405-438) on ck's device block"""
    pos, opacity, shs = ck.get_xyz, ck.get_opacity, ck.get_features
    cov = ck.get_covariance()
    mask = opacity[:, 0] > cfg["opacity_threshold"]
    init_pos, init_cov, init_opacity, init_shs = pos[mask, :], cov[mask, :], opacity[mask, :], shs[mask, :]
    rotated = init_pos
    for R in rots:
        rotated = torch.mm(rotated, R.T)
    b = cfg["sim_area"]
    mask = torch.ones(rotated.shape[0], dtype=torch.bool, device=rotated.device)
    for i in range(3):
        mask &= (rotated[:, i] > b[2 * i]) & (rotated[:, i] < b[2 * i + 1])
    unselected = (init_pos[~mask, :], init_cov[~mask, :], init_opacity[~mask, :], init_shs[~mask, :])
    rotated, init_cov, init_opacity, init_shs = rotated[mask, :], init_cov[mask, :], init_opacity[mask, :], init_shs[mask, :]
    lo, hi = torch.min(rotated, 0)[0], torch.max(rotated, 0)[0]
    scale = 1.0 / torch.max(hi - lo)
    mean = (lo + hi) / 2.0
    new_pos = (rotated - mean) * scale + torch.tensor([1.0, 1.0, 1.0], device=rotated.device) + \
        torch.tensor([0.0, 0.0, cfg["z_shift_value"]], device=rotated.device)
    c = init_cov
    full = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], dim=1).view(-1, 3, 3)
    for R in rots:
        full = torch.matmul(R, torch.matmul(full, R.T))
    f = full.reshape(-1, 9)
    new_cov = torch.stack([f[:, 0], f[:, 1], f[:, 2], f[:, 4], f[:, 5], f[:, 8]], dim=1) * (scale ** 2)
    return new_pos, new_cov, init_opacity, init_shs, unselected


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 350000])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_ingest_table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_ingest: no HIP device is visible; this measurement has no CPU form")
    dev = torch.device("cuda:0")
    rows = []
    for n in args.sizes:
        ck = checkpoint(n, 16, n)
        ck.device_block(dev)
        rots = generate_rotation_matrices(CFG["rotation_degree"], CFG["rotation_axis"], device=dev)
        routes = {"ingest_scene (HIP)": lambda: ingest_scene(ck, CFG, device=dev), "torch expressions": lambda: torch_span(ck, CFG, rots)}
        times = {k: [] for k in routes}
        for it in range(args.warmup + args.reps):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        scene = routes["ingest_scene (HIP)"]()
        n_un = scene.unselected[0].shape[0] if scene.unselected is not None else 0
        moved = n * ck.block.shape[1] * 4 + n * 16 + (scene.gs_num + n_un) * (3 + 6 + 1 + 48) * 4    # block read by emit + classify's 4 columns + outputs
        for name, ts in times.items():
            med = statistics.median(ts)
            rows.append(f"{n:>8} {name:<20} median {med:8.3f} ms   min {min(ts):8.3f}   max {max(ts):8.3f}   "
                        + (f"{moved / med / 1e6:7.1f} GB/s of {moved / 1e6:.1f} MB (block + outputs, whole call)" if "HIP" in name else ""))
        rows.append(f"{n:>8} selected {scene.gs_num}, unselected {n_un}, dropped {scene.n_dropped}")
    head = [f"scene ingest, SH degree 3 (62 columns), 2 rotations, sim_area; {args.reps} timed calls after {args.warmup} warm-up, routes alternating;",
            "host clock around one call + device synchronise (so launch overhead and the call's own synchronise are inside);",
            f"device: {torch.cuda.get_device_name(0)}", ""]
    text = "\n".join(head + rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
