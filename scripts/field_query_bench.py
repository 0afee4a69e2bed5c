#!/usr/bin/env python
"""Times the NeRF feature-field voxeliser (pixie_amd/field_query.py) against the same expression as torch ops and writes a table
(default profiles/field_query_table.txt); recorded, not asserted.  With --parity it writes instead the distances of the kernels and
of the float32 NumPy evaluation to the float64 restatement on the tests' cases (default profiles/field_query_parity.txt).

Networks: the reference's configuration with random parameters in the tiny-cuda-nn grid convention -- density net 16 levels x 2
features, 16 -> 2048, 2^19 rows per level, one hidden layer, 1 + 15 outputs (nerfacto_field.py:134-146); colour head 15 -> 64 -> 64
-> 3; feature net 12 levels x 8 features, 16 -> 128, 2^19, 6 frequencies, 64 -> 64 -> 768 (f3rm/feature_field.py:47-82).  Lattices
of 64^3 and 128^3 voxels over [-0.5, 0.5]^3, scene contraction, alpha-weighted, all arrays resident on the device.
  * fused: one FeatureFieldQuery.voxelize call (two launches; includes the output allocations).
  * torch, one batch: the same expression -- positions, contraction, selector, hash-grid gathers and blends, frequency block, the
    three MLPs as matmuls, alpha weighting, float16 casts -- as torch ops on the same device over the whole lattice at once.
  * torch, 4096 per batch: the reference's batching (voxelize.py:93-117) of that expression, results written into device arrays:
    without its three device-to-host copies and its empty_cache() per batch, so it flatters the reference.
  * floor: the float16 output bytes (C + 1 + 3 per voxel) at 6.3 TB/s.
Method: every pair alternates in the same process after `--warmup` rounds; each sample is HIP events around one call; the table
gives the median over `--reps` samples and the spread.
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pixie_amd import field_query as FQ  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
DEV = "cuda:0"


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(candidates, warmup, reps):
    for _ in range(warmup):
        for fn in candidates.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in candidates}
    for _ in range(reps):
        for name, fn in candidates.items():
            times[name].append(sample(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def random_network(gen, levels, rows, F, n_freq, n_extra, n_hidden, out_dim, act="none"):
    in_dim = (len(levels) * F if levels is not None else 0) + 6 * n_freq + n_extra
    dims = [in_dim] + [64] * n_hidden + [out_dim]
    weights = [torch.randn((dims[i + 1], dims[i]), generator=gen, device=DEV) * math.sqrt(2.0 / dims[i]) for i in range(len(dims) - 1)]
    biases = [0.1 * torch.randn(dims[i + 1], generator=gen, device=DEV) for i in range(len(dims) - 1)]
    table = torch.rand((rows, F), generator=gen, device=DEV) * 2 - 1 if levels is not None else None
    return FQ.HashMLP(levels, table, weights, biases, n_freq, n_extra, act, device=DEV)


def reference_field(gen, feature_dim=768):
    dl, drows = FQ.tcnn_levels(16, 16, FQ.growth_factor(16, 16, 2048), 19)
    fl, frows = FQ.tcnn_levels(12, 16, FQ.growth_factor(12, 16, 128), 19)
    density = random_network(gen, dl, drows, 2, 0, 0, 1, 16)
    color = random_network(gen, None, 0, 0, 0, 15, 2, 3, "sigmoid")
    feature = random_network(gen, fl, frows, 8, 6, 0, 2, feature_dim)
    return FQ.FeatureFieldQuery(density, color, feature, None, True)


# ---- the same expression as torch ops ------------------------------------------------------------------------------------------
def torch_encode(net, p):
    cols = []
    M = 0xFFFFFFFF
    for lv in net.levels:
        q = p * float(lv["scale"]) + float(lv["shift"])
        c0 = torch.floor(q)
        w = q - c0
        c0 = c0.to(torch.int64)
        acc = 0
        for corner in range(8):
            o = [corner & 1, (corner >> 1) & 1, (corner >> 2) & 1]
            x, y, z = ((c0[:, a] + o[a]) & M for a in range(3))
            res = int(lv["res"])
            idx = ((x + y * res + z * res * res) & M) if lv["dense"] else (x ^ ((y * 2654435761) & M) ^ ((z * 805459861) & M))
            idx = idx % int(lv["size"]) + int(lv["offset"])
            wt = 1
            for a in range(3):
                wt = wt * (w[:, a] if o[a] else 1 - w[:, a])
            acc = acc + wt[:, None] * net.table[idx]
        cols.append(acc)
    if net.n_frequencies:
        octaves = (2.0 ** torch.arange(net.n_frequencies, device=p.device)) * math.pi
        arg = (p[:, :, None] * octaves).reshape(len(p), 3, net.n_frequencies, 1)
        cols.append(torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1).reshape(len(p), -1))
    return torch.cat(cols, dim=1)


def torch_mlp(net, x):
    for i, (w, b) in enumerate(zip(net.weights, net.biases)):
        x = torch.addmm(b, x, w.t()) if b is not None else x @ w.t()
        if i < len(net.weights) - 1:
            x = torch.relu(x)
    return torch.sigmoid(x) if net.out_activation == 1 else x


def torch_field(field, x, voxel_size, alpha_weighted=True):
    A = torch.from_numpy(field.world_to_nerf).to(x.device)
    p = x @ A[:, :3].t() + A[:, 3]
    mag = p.abs().amax(dim=1, keepdim=True)
    p = torch.where(mag < 1, p, (2 - 1 / mag) * (p / mag))
    p = (p + 2.0) / 4.0
    sel = ((p > 0) & (p < 1)).all(dim=1, keepdim=True)
    h = torch_mlp(field.density, torch_encode(field.density, p * sel))
    density = torch.exp(h[:, :1]) * sel
    alpha = 1 - torch.exp(-density * voxel_size)
    rgb = torch_mlp(field.color, h[:, 1:])
    feature = torch_mlp(field.feature, torch_encode(field.feature, p))
    if alpha_weighted:
        feature = alpha * feature
    return feature.to(torch.float16), alpha.to(torch.float16), rgb.to(torch.float16)


def torch_batched(field, x, voxel_size, batch=4096):
    n = len(x)
    f = torch.empty((n, field.feature_dim), dtype=torch.float16, device=x.device)
    a = torch.empty((n, 1), dtype=torch.float16, device=x.device)
    c = torch.empty((n, 3), dtype=torch.float16, device=x.device)
    for i in range(0, n, batch):
        f[i:i + batch], a[i:i + batch], c[i:i + batch] = torch_field(field, x[i:i + batch], voxel_size)
    return f, a, c


def timing(args):
    gen = torch.Generator(device=DEV).manual_seed(0)
    field = reference_field(gen)
    lines = [f"NeRF feature-field voxeliser, reference configuration, {torch.cuda.get_device_name(0)}; ms, median (min .. max) of {args.reps} samples",
             f"{'lattice':>8} {'fused':>24} {'torch, one batch':>26} {'torch, 4096 per batch':>28} {'floor':>8} {'fused/floor':>12} {'one batch/fused':>16}"]
    for side in args.sides:
        vs = 1.0 / side
        lo, hi = (-0.5,) * 3, (0.5 - vs / 2,) * 3
        axes = [a.to(DEV) for a in FQ.lattice_axes(lo, hi, vs)]
        x = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
        assert len(x) == side ** 3
        got = field.voxelize(lo, hi, vs)
        want = torch_field(field, x, vs)
        worst = max(float((g.float().reshape(w.shape) - w.float()).abs().max()) for g, w in zip(got, want))
        cands = {"fused": lambda: field.voxelize(lo, hi, vs), "one": lambda: torch_field(field, x, vs)}
        if side <= args.batched_up_to:
            cands["batched"] = lambda: torch_batched(field, x, vs)
        t = alternate(cands, args.warmup, args.reps)
        floor = side ** 3 * (field.feature_dim + 4) * 2 / HBM_BYTES_PER_S * 1e3
        cell = lambda k: f"{t[k][0]:9.3f} ({t[k][1]:.3f} .. {t[k][2]:.3f})" if k in t else "not run"
        lines.append(f"{side:>6}^3 {cell('fused'):>24} {cell('one'):>26} {cell('batched'):>28} {floor:8.3f} {t['fused'][0] / floor:12.2f} {t['one'][0] / t['fused'][0]:16.2f}")
        lines.append(f"          largest |fused - torch| over the three float16 grids: {worst:.3e}")
    return lines


def parity():
    from tests import test_field_query_hip as T
    from tests import _field_query_ref as R
    lines = ["distance to the float64 restatement (tests/_field_query_ref.py), max over the array: kernel, float32 NumPy, ratio, bar",
             f"{'case':<44} {'kernel':>11} {'float32':>11} {'ratio':>7} {'bar':>11}"]

    def row(what, got, ref, f32, nets):
        err, yard = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(f32.astype(np.float64) - ref).max())
        lines.append(f"{what:<44} {err:11.3e} {yard:11.3e} {err / yard if yard else float('inf'):7.2f} {R.bar(ref, f32, nets):11.3e}")

    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    for name in T.NETS:
        net, p, extra, ref, f32 = T.case(name)
        got = T.device_net(net)(t(p) if net["levels"] else None, t(extra))
        row(name, got.cpu().numpy(), ref, f32, [net])
    for name in T.LATTICES:
        fq, x, shape, ref, f32 = T.lattice_case(name)
        lo, hi, vs, _, _, weighted, _ = T.LATTICES[name]
        field = T.device_field(fq)
        _, _, _, density, alpha32 = field.voxelize(lo, hi, vs, weighted, return_density=True, return_alpha32=True)
        pts = t(x)
        row(f"{name} density", density.cpu().numpy().reshape(-1), ref["density"], f32["density"], [fq["density"]])
        row(f"{name} alpha", alpha32.cpu().numpy().reshape(-1), ref["alpha"], f32["alpha"], [fq["density"]])
        row(f"{name} feature", field(pts)["feature"].cpu().numpy(), ref["feature"], f32["feature"], [fq["feature"]])
        row(f"{name} rgb", field.get_rgb(pts).cpu().numpy(), ref["rgb"], f32["rgb"], [fq["density"], fq["color"]])
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--batched-up-to", type=int, default=128, help="largest lattice side for which the 4096-per-batch loop is timed")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = parity() if args.parity else timing(args)
    out = args.out or os.path.join(REPO, "profiles", "field_query_parity.txt" if args.parity else "field_query_table.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
