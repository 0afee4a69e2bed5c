#!/usr/bin/env python
"""Times the part segmentation (pixie_amd/part_segmentation.py) against the reference's route and writes a table (default
profiles/part_segmentation_table.txt); recorded, not asserted.  With --parity it also writes the score distances of the kernel and of
the float32 torch expression to the float64 restatement on the tests' scenes (default profiles/part_segmentation_parity.txt).

Method (scripts/train_step_bench.py's): every pair (ours, torch) alternates in the same process, `--warmup` rounds of both first;
each sample is HIP events around `--inner` back-to-back calls; the table gives the median over `--reps` samples and the spread.
  * stage A rows: one part_segmentation call (work list, scores, labels, counts, no material grid) against segmentation.py:77-80,
    103-120, 164-168 as torch ops on the same device -- the masked gather, the widening to float32, both normalisations, the
    matmul, the softmax, argmax and gather -- with the feature grid already on the device for both.  64^3 x 768 with a ball of about
    17 k masked voxels and 128^3 x 768 with about 124 k, K = 5.  The floor is the row traffic alone, n 2 C bytes at 6.3 TB/s.
  * stage B rows: the same call with smooth_k = 200 (the whole call is timed, stage A included, on one-hot 8-channel features so
    that stage A is negligible) against local_post_process_segmentation's loop -- one KDTree.query and one
    scipy.stats.mode per voxel -- on the HOST, for the first `--host-voxels` voxels only and scaled to all of them, which the row says.
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
from pixie_amd.part_segmentation import part_segmentation  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(candidates, warmup, reps, inner):
    for _ in range(warmup):
        for fn in candidates.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in candidates}
    for _ in range(reps):
        for name, fn in candidates.items():
            times[name].append(sample(fn, inner))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def torch_stage_a(features, mask, queries, temperature=0.1):
    features_flat = features.reshape(-1, features.shape[-1])
    features_filtered = features_flat[mask.reshape(-1)]
    features_filtered = features_filtered.to(torch.float32)
    features_filtered /= features_filtered.norm(dim=-1, keepdim=True)
    query_embs = queries.float().clone()
    query_embs /= query_embs.norm(dim=-1, keepdim=True)
    similarities = features_filtered @ query_embs.T
    probabilities = torch.nn.functional.softmax(similarities / temperature, dim=1)
    part_labels = torch.argmax(probabilities, dim=1)
    return part_labels, torch.gather(probabilities, 1, part_labels.unsqueeze(1)).squeeze(1)


def ball_mask(size, fraction, dev):
    r = torch.arange(size, device=dev, dtype=torch.float32) - (size - 1) / 2
    radius = (fraction * size ** 3 * 3 / (4 * np.pi)) ** (1 / 3)
    return (r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2) <= radius ** 2


def host_vote_seconds(mask, labels, k, voxels):
    from scipy.stats import mode
    from sklearn.neighbors import KDTree
    axes = [np.linspace(-0.5, 0.5, s, dtype=np.float32) for s in mask.shape]
    idx = np.argwhere(mask)
    coords = np.stack([axes[a][idx[:, a]] for a in range(3)], axis=1)
    tree = KDTree(coords)
    t0 = time.perf_counter()
    for i in range(voxels):
        _, nearest = tree.query(coords[i].reshape(1, -1), k=k)
        mode(labels[nearest[0]], keepdims=False)
    return (time.perf_counter() - t0) / voxels


def parity_lines():
    from tests import _part_seg_ref as R
    lines = ["score distance to the float64 restatement on the tests' scenes: worst |score - score64| over the masked voxels",
             f"{'scene':10s} {'voxels':>7s} {'inside tau':>10s} {'kernel':>11s} {'torch fp32 (cpu)':>17s} {'bar':>11s} {'labels differ (kernel / torch)':>31s}"]
    for name in R.STAGE_A:
        if name == "empty":
            continue
        sc = R.stage_a_scene(name)
        ref = R.stage_a64(sc["features"], sc["mask"], sc["queries"])
        seg = part_segmentation(torch.from_numpy(sc["features"]).cuda(), torch.from_numpy(sc["mask"]).cuda(), sc["queries"])
        t_labels, t_scores = R.stage_a_torch(sc["features"], sc["mask"], sc["queries"])
        fine = ~np.isnan(ref["scores"])
        ours = np.abs(seg.part_scores.cpu().numpy().astype(np.float64)[fine] - ref["scores"][fine]).max()
        theirs = np.abs(t_scores.astype(np.float64)[fine] - ref["scores"][fine]).max()
        channels = sc["features"].shape[-1]
        lines.append(f"{name:10s} {int(sc['mask'].sum()):7d} {int((ref['margin'] <= R.tau(channels)).sum()):10d} {ours:11.3e} {theirs:17.3e} "
                     f"{R.score_bar(channels):11.3e} {int((seg.part_labels.cpu().numpy() != ref['labels']).sum()):15d} / {int((t_labels != ref['labels']).sum()):d}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "part_segmentation_table.txt"))
    ap.add_argument("--parity", nargs="?", const=os.path.join(REPO, "profiles", "part_segmentation_parity.txt"), default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-voxels", type=int, default=300)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    props = torch.cuda.get_device_properties(0)
    lines = [f"part segmentation on {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs): median ms over {args.reps} samples of {args.inner} back-to-back calls (min .. max), "
             "candidates alternating", ""]
    channels, parts = 768, 5
    for size in args.sizes:
        mask = ball_mask(size, 0.065 if size == 64 else 0.059, dev)
        n = int(mask.sum())
        features = (torch.randn((size, size, size, channels), generator=gen, device=dev, dtype=torch.float32) / channels ** 0.5).half()
        queries = torch.randn((parts, channels), generator=gen, device=dev)
        t = alternate({"ours": lambda: part_segmentation(features, mask, queries),
                       "torch": lambda: torch_stage_a(features, mask, queries)}, args.warmup, args.reps, args.inner)
        floor_ms = n * 2 * channels / HBM_BYTES_PER_S * 1e3
        lines.append(f"stage A  {size}^3 x {channels}, K = {parts}, {n} masked voxels; row-traffic floor n 2 C / 6.3 TB/s = {floor_ms:.4f} ms")
        for name in ("ours", "torch"):
            med, lo, hi = t[name]
            lines.append(f"    {name:6s} {med:9.4f} ms  ({lo:.4f} .. {hi:.4f})")
        lines.append(f"    torch / ours = {t['torch'][0] / t['ours'][0]:.2f}")
        del features

        labels = (torch.arange(size, device=dev)[None, :, None] * 6 // size).expand(size, size, size).clone()
        labels[torch.rand((size, size, size), generator=gen, device=dev) < 0.04] = 0
        one_hot = torch.zeros((size, size, size, 8), dtype=torch.float16, device=dev)
        one_hot.scatter_(3, labels[..., None], 1.0)
        eye = torch.eye(6, 8, device=dev)
        t = alternate({"ours": lambda: part_segmentation(one_hot, mask, eye, smooth_k=200)}, args.warmup, args.reps, args.inner)
        seg = part_segmentation(one_hot, mask, eye, smooth_k=200)
        voxels = min(args.host_voxels, n)
        per_voxel = host_vote_seconds(mask.cpu().numpy(), labels[mask].cpu().numpy(), 200, voxels)
        med, lo, hi = t["ours"]
        lines.append(f"stage B  {size}^3, k = 200, {n} masked voxels, {seg.slow_path_voxels} on the slow path (whole call, stage A on 8 channels included)")
        lines.append(f"    ours   {med:9.4f} ms  ({lo:.4f} .. {hi:.4f})")
        lines.append(f"    host   {per_voxel * n * 1e3:9.1f} ms  sklearn KDTree.query + scipy.stats.mode per voxel: {per_voxel * 1e6:.0f} us per voxel measured on the "
                     f"first {voxels} voxels only, scaled to {n}")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if args.parity:
        parity = parity_lines()
        with open(args.parity, "w") as f:
            f.write("\n".join(parity) + "\n")
        print("\n".join(parity))


if __name__ == "__main__":
    main()
