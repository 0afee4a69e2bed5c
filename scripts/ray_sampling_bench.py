#!/usr/bin/env python
"""Times proposal sampling and its two losses through pixie_amd.ray_sampling against the reference's lines as torch ops
(tests/_ray_sampling_ref.py) on the same device, and writes a table (default profiles/ray_sampling_table.txt); recorded, not asserted.

Shape: R = 4096 rays, levels (256, 96, 48), single jitter (f3rm's nerfacto settings), annealing exponent 1 and 0.5.
  * the three sampler calls one by one: piecewise 256; pdf 256 -> 96; pdf 96 -> 48 (positions included on our side, as the density_fn
    reads them next; the torch side computes get_positions too).
  * each loss forward + backward: interlevel over the two proposal levels, distortion on the fine level.
  * the whole span: ProposalNetworkSampler with two analytic density_fns (a Gaussian blob with a learnable height), fine weights from
    the second, interlevel + 0.002 distortion, backward.  The density_fns and get_weights (ray_render's kernel on our side, torch ops
    on the other) are inside both spans.
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
from field_query_bench import DEV, alternate  # noqa: E402
from pixie_amd import ray_sampling as rs  # noqa: E402
from tests import _ray_sampling_ref as ref  # noqa: E402


class Blob(torch.nn.Module):
    def __init__(self, height, centre):
        super().__init__()
        self.height = torch.nn.Parameter(torch.tensor(float(height), device=DEV))
        self.centre = torch.tensor(centre, dtype=torch.float32, device=DEV)

    def forward(self, positions):
        return (torch.nn.functional.softplus(self.height) * torch.exp(-((positions - self.centre) ** 2).sum(-1, keepdim=True) * 0.5) * 4.0).contiguous()


def make_bundle(gen, n_rays):
    rand = lambda *s: torch.rand(s, generator=gen, device=DEV)
    d = torch.randn((n_rays, 3), generator=gen, device=DEV)
    return SimpleNamespace(origins=rand(n_rays, 3) * 2 - 1, directions=d / d.norm(dim=1, keepdim=True), nears=rand(n_rays, 1) * 0.45 + 0.05,
                           fars=rand(n_rays, 1) * 4 + 2, pixel_area=rand(n_rays, 1) * 1e-5)


def ours_span(sampler, bundle, fns):
    for fn in fns:
        fn.height.grad = None
    samples, weights_list, samples_list = sampler(bundle, fns)
    weights_list, samples_list = weights_list + [samples.get_weights(fns[-1](samples.frustums.get_positions()))], samples_list + [samples]
    (rs.interlevel_loss(weights_list, samples_list) + 0.002 * rs.distortion_loss(weights_list, samples_list)).backward()


def torch_span(bundle, fns, levels, n_fine, anneal):
    for fn in fns:
        fn.height.grad = None
    samples, weights_list, samples_list = ref.proposal_sample(bundle, fns, levels, n_fine, True, True, DEV, anneal=anneal)
    weights_list, samples_list = weights_list + [ref.get_weights(samples, fns[-1](samples.frustums.get_positions()))], samples_list + [samples]
    (ref.interlevel_loss(weights_list, samples_list) + 0.002 * ref.distortion_loss(weights_list, samples_list)).backward()


def loss_pass(fn, weights_list, samples_list):
    for w in weights_list:
        w.grad = None
    fn(weights_list, samples_list).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--levels", type=int, nargs=2, default=[256, 96])
    ap.add_argument("--fine", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ray_sampling_table.txt"))
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    R, levels, n_fine = args.rays, tuple(args.levels), args.fine
    bundle = make_bundle(gen, R)
    fns = [Blob(1.0, (0.2, -0.1, 0.3)), Blob(0.5, (-0.3, 0.4, 0.0))]
    cell = lambda v: f"{v[0]:8.3f} ({v[1]:.3f} .. {v[2]:.3f})"
    lines = [f"proposal sampling and its losses, {torch.cuda.get_device_name(0)}; ms, median (min .. max) of {args.reps} samples",
             f"R = {R}, levels {levels + (n_fine,)}, single jitter; ours = pixie_amd.ray_sampling, torch = tests/_ray_sampling_ref.py on the device"]

    def row(name, v):
        lines.append(f"{name:>44}  ours {cell(v['ours']):>30}  torch {cell(v['torch']):>30}  torch / ours {v['torch'][0] / v['ours'][0]:6.2f}")

    # the sampler calls one by one, on fixed inputs from one run of our sampler
    sampler = rs.ProposalNetworkSampler(num_proposal_samples_per_ray=levels, num_nerf_samples_per_ray=n_fine, single_jitter=True).to(DEV)
    with torch.no_grad():
        fine, weights_list, samples_list = sampler(bundle, fns)
        fine_weights = fine.get_weights(fns[-1](fine.frustums.get_positions()))
    initial, pdf = sampler.initial_sampler, sampler.pdf_sampler
    ref_level0 = ref.spaced_sample(bundle, "piecewise", levels[0], torch.rand((R, 1), device=DEV))
    row(f"piecewise sampler, {levels[0]} samples", alternate({
        "ours": lambda: initial(bundle, num_samples=levels[0]),
        "torch": lambda: ref.spaced_sample(bundle, "piecewise", levels[0], torch.rand((R, 1), device=DEV)).frustums.get_positions()},
        args.warmup, args.reps))
    sizes = levels + (n_fine,)
    for anneal in (1.0, 0.5):
        for k in (1, 2):
            existing, w = samples_list[k - 1], weights_list[k - 1]
            ref_existing = SimpleNamespace(spacing_starts=existing.spacing_starts, spacing_ends=existing.spacing_ends,
                                           spacing_to_euclidean_fn=ref_level0.spacing_to_euclidean_fn)
            row(f"pdf sampler {sizes[k - 1]} -> {sizes[k]}, anneal {anneal:g}", alternate({
                "ours": lambda: pdf(bundle, existing, w, num_samples=sizes[k], anneal=anneal),
                "torch": lambda: ref.pdf_sample(bundle, ref_existing, torch.pow(w, anneal), sizes[k], torch.rand((R, 1), device=DEV), False)
                .frustums.get_positions()}, args.warmup, args.reps))
    all_weights = [w.detach().clone().requires_grad_(True) for w in weights_list + [fine_weights]]
    all_samples = samples_list + [fine]
    row("interlevel loss forward + backward", alternate({"ours": lambda: loss_pass(rs.interlevel_loss, all_weights, all_samples),
                                                         "torch": lambda: loss_pass(ref.interlevel_loss, all_weights, all_samples)},
                                                        args.warmup, args.reps))
    row("distortion loss forward + backward", alternate({"ours": lambda: loss_pass(rs.distortion_loss, all_weights[-1:], all_samples[-1:]),
                                                         "torch": lambda: loss_pass(ref.distortion_loss, all_weights[-1:], all_samples[-1:])},
                                                        args.warmup, args.reps))
    for anneal in (1.0, 0.5):
        sampler.set_anneal(anneal)
        row(f"sampler + losses span, anneal {anneal:g}", alternate({"ours": lambda: ours_span(sampler, bundle, fns),
                                                                   "torch": lambda: torch_span(bundle, fns, levels, n_fine, anneal)},
                                                                  args.warmup, args.reps))
    lines.append("not measured: kernel times apart from the host's launches (no kernel trace was taken), other R, per-sample jitter, include_original,")
    lines.append("the eval path, and the span inside a training step with the hash-grid networks as density_fns.")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
