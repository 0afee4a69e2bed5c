#!/usr/bin/env python
"""Times one training pass (forward with saved activations + backward) of the three reference networks through
pixie_amd.field_training.TrainableHashMLP against the same expression as torch ops under autograd, and writes a table (default
profiles/hashmlp_grad_table.txt); recorded, not asserted.

Networks: the reference's configuration with random parameters in the tiny-cuda-nn grid convention, n = 196 608 uniform points (4096
rays x 48 samples, f3rm_config.py:35) -- density net 16 levels x 2 features, 16 -> 2048, 2^19 rows per level, 32 -> 64 -> 16; colour
head 15 -> 64 -> 64 -> 3, sigmoid, its 15 input columns requiring a gradient; feature net 12 levels x 8 features, 16 -> 128, 2^19, 6
frequencies, 132 -> 64 -> 64 -> 768.  dY is a fixed standard-normal array.
  * module: TrainableHashMLP forward + out.backward(dY): pixie_hashmlp_forward_saved, pixie_hashmlp_backward and the allocations
    around them (output, saved arrays, gradients, scratch, from torch's caching allocator).
  * torch: scripts/field_query_bench.py's torch_encode / torch_mlp with requires_grad parameters, out.backward(dY): one batch,
    autograd's index_put_(accumulate) table gradient (float atomics: not reproducible from run to run).
  * without table: the module with the table's requires_grad off (the scatter, its memset and the finalise do not run).
  * scatter alone: module time with dY as given minus module time with dY = 0.  With dY = 0 every launch still runs, the scatter
    kernel returns at its first branch (M == 0), so the difference is the scatter's body.  Caveat: zero operands let the matrix
    instructions run at a higher clock, which makes the dY = 0 run slightly faster than the launches it stands for and so
    overstates the scatter.  added bytes = 8 bytes x n x levels x 8 corners x features.
Per-kernel times: run it under `rocprofv3 --kernel-trace` with --no-torch and summarise the database with scripts/rocpd_stats.py
(profiles/hashmlp_grad_kernel_stats_by_geometry.csv).
Method: the candidates alternate in the same process after `--warmup` rounds; each sample is HIP events around one pass; the table
gives the median over `--reps` samples and the spread.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from field_query_bench import DEV, alternate, random_network, torch_encode, torch_mlp  # noqa: E402
from pixie_amd import field_query as FQ, field_training as FT  # noqa: E402


def networks(gen):
    dl, drows = FQ.tcnn_levels(16, 16, FQ.growth_factor(16, 16, 2048), 19)
    fl, frows = FQ.tcnn_levels(12, 16, FQ.growth_factor(12, 16, 128), 19)
    return {"density": random_network(gen, dl, drows, 2, 0, 0, 1, 16), "color": random_network(gen, None, 0, 0, 0, 15, 2, 3, "sigmoid"),
            "feature": random_network(gen, fl, frows, 8, 6, 0, 2, 768)}


def torch_pass(net, leaves, pos, extra, dY):
    for t in leaves:
        t.grad = None
    cols = [torch_encode(net, pos)] if len(net.levels) else []
    if extra is not None:
        cols.append(extra)
    torch_mlp(net, torch.cat(cols, dim=1)).backward(dY)


def module_pass(m, pos, extra, dY):
    for t in m.parameters():
        t.grad = None
    if extra is not None:
        extra.grad = None
    m(pos, extra).backward(dY)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=196608)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch baseline out (for a kernel trace of the module alone)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hashmlp_grad_table.txt"))
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    nets = networks(gen)
    n = args.n
    pos = torch.rand((n, 3), generator=gen, device=DEV)
    cell = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    lines = [f"hash-grid MLP training pass (forward saved + backward), reference networks, n = {n}, {torch.cuda.get_device_name(0)}; ms, median "
             f"(min .. max) of {args.reps} samples",
             f"{'network':>8} {'module':>26} {'torch autograd':>28} {'torch/module':>13} {'without table':>26} {'scatter alone':>14} {'share':>6} "
             f"{'added GB':>9} {'TB/s':>6} {'saved B/pt':>10}"]
    for name, h in nets.items():
        m = FT.TrainableHashMLP.from_hashmlp(h)
        extra = torch.randn((n, h.n_extra), generator=gen, device=DEV).requires_grad_(True) if h.n_extra else None
        p = pos if len(h.levels) else None
        dY = torch.randn((n, h.out_dim), generator=gen, device=DEV)
        zero = torch.zeros_like(dY)
        leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)
        twin = SimpleNamespace(levels=h.levels, table=leaf(h.table), weights=[leaf(w) for w in h.weights], biases=[leaf(b) for b in h.biases],
                               n_frequencies=h.n_frequencies, out_activation=h.out_activation)        # torch leaves of their own
        twin_leaves = [t for t in [twin.table] + twin.weights + twin.biases if t is not None]
        copy = lambda t: None if t is None else t.clone()
        frozen = FT.TrainableHashMLP.from_hashmlp(FQ.HashMLP(h.levels if len(h.levels) else None, copy(h.table), [copy(w) for w in h.weights],
                                                              [copy(b) for b in h.biases], h.n_frequencies, h.n_extra,
                                                              {0: "none", 1: "sigmoid", 2: "exp"}[h.out_activation], device=DEV))
        if frozen.table is not None:
            frozen.table.requires_grad_(False)
        cands = {"module": lambda: module_pass(m, p, extra, dY), "torch": lambda: torch_pass(twin, twin_leaves, p, extra, dY),
                 "frozen": lambda: module_pass(frozen, p, extra, dY), "zero": lambda: module_pass(m, p, extra, zero)}
        if args.no_torch:
            del cands["torch"]
        t = alternate(cands, args.warmup, args.reps)
        saved_bytes, _ = FT.train_bytes(h.desc(), n)
        versus = f"{cell(t['torch']):>28} {t['torch'][0] / t['module'][0]:13.2f}" if "torch" in t else f"{'not run':>28} {'-':>13}"
        row = f"{name:>8} {cell(t['module']):>26} {versus} {cell(t['frozen']):>26}"
        if len(h.levels):
            scatter = t["module"][0] - t["zero"][0]
            items = n * len(h.levels) * 8 * h.features_per_level          # upper count: every contribution, zero or not
            row += f" {scatter:14.3f} {scatter / t['module'][0]:6.2f} {items * 8 / 1e9:9.3f} {items * 8 / 1e12 / (scatter / 1e3):6.2f}"
        else:
            row += f" {'-':>14} {'-':>6} {'-':>9} {'-':>6}"
        lines.append(row + f" {saved_bytes // n:10d}")
    lines.append("added GB counts 8 bytes for every (point, level, corner, feature) contribution; those that quantise to zero are skipped by the kernel,")
    lines.append("so the TB/s column is an upper bound on the rate of atomics actually issued.  scatter alone and share are by difference (see the script).")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
