#!/usr/bin/env python
"""Times the proposal density field (pixie_amd.density_field) against the two other ways to run the same network on the device, and
writes a table (default profiles/density_field_table.txt); recorded, not asserted.

Workload: nerfacto's two proposal networks (5 levels x 2 features, 16 -> 128 / 256, 2^17 rows per level, one hidden layer of 16) with
random parameters, at n = 4096 x 256 and 4096 x 96 points uniform in [-3, 3]^3 under the contraction.
  (a) this path: one launch forward; backward = recompute + slab sums + fixed-point scatter
  (b) the zero-padded 64-wide twin (to_trainable_hashmlp) with torch's contraction, selector and trunc_exp around it
  (c) the reference's lines as torch ops: nerfstudio's torch hash encoding (encodings.py pytorch_fwd) + nn.Linear, restated below
Rows: the inference forward alone (under no_grad), forward + backward, (a)'s forward + backward with a zero upstream gradient (max |dX|
= 0: the scatter returns at once, so the difference is the scatter's share), and the sampler + losses span of ray_sampling_bench.py
with the two real density fields as density_fns on both sides ((a) against (c)).
Method: the candidates alternate in the same process after `--warmup` rounds; each sample is HIP events around one pass; the table
gives the median over `--reps` samples and the spread.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from field_query_bench import DEV, alternate  # noqa: E402
from pixie_amd import density_field as DF  # noqa: E402
from pixie_amd import ray_sampling as rs  # noqa: E402
from ray_sampling_bench import make_bundle  # noqa: E402
from tests import _ray_sampling_ref as ref  # noqa: E402

AID = 1.0


class TruncExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, min=-15, max=15))


def front_end(x):
    mag = x.abs().amax(dim=-1, keepdim=True)
    p = torch.where(mag < 1, x, (2 - 1 / mag) * (x / mag))
    p = (p + 2.0) / 4.0
    sel = ((p > 0.0) & (p < 1.0)).all(dim=-1)
    return p * sel[..., None], sel


class Twin(torch.nn.Module):
    """(b)"""

    def __init__(self, field):
        super().__init__()
        self.net = field.to_trainable_hashmlp()

    def forward(self, positions):
        p, sel = front_end(positions)
        h = self.net(p.reshape(-1, 3)).reshape(*positions.shape[:-1], 1)
        return AID * TruncExp.apply(h) * sel[..., None]


class TorchOps(torch.nn.Module):
    """(c): HashEncoding.pytorch_fwd's lines, then nn.Linear layers"""

    def __init__(self, field, log2_T):
        super().__init__()
        self.T = 1 << log2_T
        self.scalings = torch.tensor(field.levels["scale"], device=DEV)
        self.offsets = torch.arange(len(field.levels), device=DEV) * self.T
        self.primes = torch.tensor([1, 2654435761, 805459861], device=DEV)
        self.table = torch.nn.Parameter(field.table.detach().clone())
        self.layers = torch.nn.ModuleList()
        for w, b in zip(field.weights, field.bias_list()):
            lin = torch.nn.Linear(w.shape[1], w.shape[0], device=DEV)
            with torch.no_grad():
                lin.weight.copy_(w)
                lin.bias.copy_(b)
            self.layers.append(lin)

    def hash_fn(self, t):
        t = t * self.primes
        x = torch.bitwise_xor(torch.bitwise_xor(t[..., 0], t[..., 1]), t[..., 2])
        return x % self.T + self.offsets

    def encode(self, p):
        scaled = p[..., None, :] * self.scalings.view(-1, 1)
        c, f = torch.ceil(scaled).type(torch.int64), torch.floor(scaled).type(torch.int64)
        offset = scaled - f
        pick = lambda a, b, cc: self.table[self.hash_fn(torch.cat([a[..., 0:1], b[..., 1:2], cc[..., 2:3]], dim=-1))]
        f0, f1, f2, f3 = pick(c, c, c), pick(c, f, c), pick(f, f, c), pick(f, c, c)
        f4, f5, f6, f7 = pick(c, c, f), pick(c, f, f), pick(f, f, f), pick(f, c, f)
        f03 = f0 * offset[..., 0:1] + f3 * (1 - offset[..., 0:1])
        f12 = f1 * offset[..., 0:1] + f2 * (1 - offset[..., 0:1])
        f56 = f5 * offset[..., 0:1] + f6 * (1 - offset[..., 0:1])
        f47 = f4 * offset[..., 0:1] + f7 * (1 - offset[..., 0:1])
        f0312 = f03 * offset[..., 1:2] + f12 * (1 - offset[..., 1:2])
        f4756 = f47 * offset[..., 1:2] + f56 * (1 - offset[..., 1:2])
        return torch.flatten(f0312 * offset[..., 2:3] + f4756 * (1 - offset[..., 2:3]), start_dim=-2, end_dim=-1)

    def forward(self, positions):
        p, sel = front_end(positions)
        x = self.encode(p.reshape(-1, 3))
        for i, lin in enumerate(self.layers):
            x = lin(x)
            if i < len(self.layers) - 1:
                x = torch.relu(x)
        return AID * TruncExp.apply(x.reshape(*positions.shape[:-1], 1)) * sel[..., None]


def train_pass(module, x, g):
    for p in module.parameters():
        p.grad = None
    module(x).backward(g)


def infer_pass(module, x):
    with torch.no_grad():
        module(x)


def span(sample, weights_of, fns):
    for fn in fns:
        for p in fn.parameters():
            p.grad = None
    samples, weights_list, samples_list = sample()
    weights_list = weights_list + [weights_of(samples, fns[-1](samples.frustums.get_positions()))]
    samples_list = samples_list + [samples]
    return weights_list, samples_list


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--levels", type=int, nargs=2, default=[256, 96])
    ap.add_argument("--fine", type=int, default=48)
    ap.add_argument("--log2-hashmap-size", type=int, default=17)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "density_field_table.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    R, levels, T = args.rays, tuple(args.levels), args.log2_hashmap_size
    ours = []
    for max_res in (128, 256):
        f = DF.HashMLPDensityField(None, num_layers=2, hidden_dim=16, spatial_distortion=True, num_levels=5, max_res=max_res, base_res=16,
                                   log2_hashmap_size=T, features_per_level=2, average_init_density=AID, implementation="torch", device=DEV)
        with torch.no_grad():
            f.table.copy_(torch.rand(f.table.shape, generator=gen, device=DEV) * 2 - 1)
        ours.append(f)
    twins, ops = [Twin(f) for f in ours], [TorchOps(f, T) for f in ours]
    cell = lambda v: f"{v[0]:8.3f} ({v[1]:.3f} .. {v[2]:.3f})"
    lines = [f"proposal density fields, {torch.cuda.get_device_name(0)}; ms, median (min .. max) of {args.reps} samples",
             f"5 x F2 levels, 16 -> 128 / 256, T = 2^{T}, one hidden layer of 16; (a) pixie_amd.density_field, (b) the zero-padded 64-wide twin "
             "with torch front and back ends, (c) torch ops"]

    def row(name, v):
        a = v["a"][0]
        lines.append(f"{name:>52}  (a) {cell(v['a']):>28}  (b) {cell(v['b']):>28}  (c) {cell(v['c']):>28}  b / a {v['b'][0] / a:6.2f}  c / a {v['c'][0] / a:6.2f}")

    for k, S in enumerate(levels):
        n = R * S
        x = torch.rand((n, 3), generator=gen, device=DEV) * 6 - 3
        g = torch.randn((n, 1), generator=gen, device=DEV)
        mods = {"a": ours[k], "b": twins[k], "c": ops[k]}
        row(f"network {k} (max_res {(128, 256)[k]}), n = {R} x {S}: inference forward",
            alternate({name: (lambda m=m: infer_pass(m, x)) for name, m in mods.items()}, args.warmup, args.reps))
        row(f"network {k}, n = {R} x {S}: forward + backward",
            alternate({name: (lambda m=m: train_pass(m, x, g)) for name, m in mods.items()}, args.warmup, args.reps))
        zero = torch.zeros_like(g)
        v = alternate({"dY": lambda: train_pass(ours[k], x, g), "dY = 0": lambda: train_pass(ours[k], x, zero)}, args.warmup, args.reps)
        lines.append(f"{'(a) forward + backward, upstream = 0':>52}  {cell(v['dY = 0'])} against {cell(v['dY'])}: the scatter's share "
                     f"{(v['dY'][0] - v['dY = 0'][0]) / v['dY'][0]:.2f}")
    bundle = make_bundle(gen, R)
    sampler = rs.ProposalNetworkSampler(num_proposal_samples_per_ray=levels, num_nerf_samples_per_ray=args.fine, single_jitter=True).to(DEV)

    def ours_span():
        weights_list, samples_list = span(lambda: sampler(bundle, [f.density_fn for f in ours]), lambda s, d: s.get_weights(d), ours)
        (rs.interlevel_loss(weights_list, samples_list) + 0.002 * rs.distortion_loss(weights_list, samples_list)).backward()

    def torch_span():
        weights_list, samples_list = span(lambda: ref.proposal_sample(bundle, ops, levels, args.fine, True, True, DEV, anneal=1.0), ref.get_weights, ops)
        (ref.interlevel_loss(weights_list, samples_list) + 0.002 * ref.distortion_loss(weights_list, samples_list)).backward()

    v = alternate({"a": ours_span, "c": torch_span}, args.warmup, args.reps)
    lines.append(f"{'sampler + losses span with the real density fields':>52}  (a) {cell(v['a']):>28}  (c) {cell(v['c']):>28}  c / a {v['c'][0] / v['a'][0]:6.2f}")
    lines.append("not measured: kernel times apart from the host's launches (no kernel trace was taken), a lane per (point, corner) gather mapping,")
    lines.append("a backward that reads saved activations instead of recomputing, other table sizes, F = 4 / 8, two hidden layers, use_linear.")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
