#!/usr/bin/env python
"""Times what gaussian-splatting/train.py does with the gradients of an iteration -- the optimiser step, the densification
statistics and densify_and_prune (pixie_amd/gaussian_optim.py) -- against the same work as torch ops on the same device, and one
whole training iteration (render, fused loss, backward, statistics, step) with either optimiser.  Writes a table (default
profiles/train_optim_table.txt); recorded, not asserted.

Method (that of scripts/train_step_bench.py): every pair alternates in the same process after `--warmup` rounds of both; each
sample is HIP events around `--inner` back-to-back iterations; the table gives the median over `--reps` samples and the spread.
  * Adam rows, 100 k and 350 k Gaussians at SH degree 3 (59 floats each): GaussianAdam.step() against torch.optim.Adam as the
    reference constructs it (scene/gaussian_model.py:163: six one-tensor groups, lr=0.0, eps=1e-15) and, separately, against
    torch.optim.Adam(fused=True), which the reference does not use.  The kernel moves 7 x 4 B x 59 = 1652 B per Gaussian; the row
    gives the measured time as a multiple of that traffic at 6.3 TB/s.
  * statistics rows: one pixie_gs_densify_stats launch against the three masked torch lines of train.py:114-116.
  * densify rows: densify_and_prune against a torch restatement of gaussian_model.py:353-405 on the same device (clone, split and
    two prunes as cat / masked gathers over the six parameters and twelve moments), wall time including their synchronises.
  * iteration rows: GaussianRasterizer at `--gaussians` Gaussians (shs, degree 3), 800 x 800, fused photometric loss, backward,
    statistics, optimiser step.
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
from pixie_amd import gaussian_optim as go  # noqa: E402
from pixie_amd.losses import photometric_loss  # noqa: E402
from pixie_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from scripts.raster_bench import look_at_camera  # noqa: E402
from scripts.train_step_bench import alternate, fmt  # noqa: E402

LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
HBM_BYTES_PER_S = 6.3e12          # the achievable rate the microarchitecture guide gives
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY = 5.0, 0.01, 0.0002, 0.005


def population(n, dev, seed=0, scales=(2e-3, 8e-3)):
    """six parameters of a plausible scene: positions in a ball, scales around the densification thresholds, mixed opacities"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    prob = rng.uniform(0.001, 0.99, n)
    return {"xyz": t(d * (0.5 * rng.random(n) ** (1 / 3))[:, None]), "f_dc": t(rng.normal(0, 1, (n, 1, 3))), "f_rest": t(rng.normal(0, 0.1, (n, 15, 3))),
            "opacity": t(np.log(prob / (1 - prob))[:, None]), "scaling": t(rng.uniform(np.log(scales[0]), np.log(scales[1]), (n, 3))), "rotation": t(rng.normal(0, 1, (n, 4)))}


def groups(params):
    return [{"params": [torch.nn.Parameter(params[f].clone())], "lr": LRS[f], "name": f} for f in go.FIELDS]


def adam_rows(a, dev, lines):
    for n in (100_000, 350_000):
        base = population(n, dev)
        opts = {"hip": go.GaussianAdam(groups(base), lr=0.0, eps=1e-15), "torch": torch.optim.Adam(groups(base), lr=0.0, eps=1e-15),
                "torch_fused": torch.optim.Adam(groups(base), lr=0.0, eps=1e-15, fused=True)}
        gen = torch.Generator(device=dev).manual_seed(n)
        grads = [torch.randn(base[f].shape, generator=gen, device=dev) * 1e-3 for f in go.FIELDS]
        for opt in opts.values():
            for g, grad in zip(opt.param_groups, grads):
                g["params"][0].grad = grad
        tm = alternate({k: o.step for k, o in opts.items()}, a.warmup, a.reps, a.inner)
        floor_us = 7 * 4 * 59 * n / HBM_BYTES_PER_S * 1e6
        med = {k: statistics.median(v) for k, v in tm.items()}
        lines.append(f"Adam step, {n} Gaussians x 59 floats:  GaussianAdam {fmt(tm['hip'])}   torch.optim.Adam (reference's) {fmt(tm['torch'])}   "
                     f"torch.optim.Adam(fused=True) {fmt(tm['torch_fused'])}   ratio to reference's {med['torch'] / med['hip']:.2f}, to fused "
                     f"{med['torch_fused'] / med['hip']:.2f}   traffic floor {floor_us:.1f} us at 6.3 TB/s: measured = {med['hip'] * 1e3 / floor_us:.2f} x floor")


def torch_stats(accum, denom, max_radii2D, vgrad, radii):
    vis = radii > 0
    max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis])
    accum[vis] += torch.norm(vgrad[vis, :2], dim=-1, keepdim=True)
    denom[vis] += 1


def stats_rows(a, dev, lines):
    for n in (100_000, 350_000):
        gen = torch.Generator(device=dev).manual_seed(n)
        vgrad = torch.randn((n, 3), generator=gen, device=dev) * 1e-4
        radii = (torch.rand((n,), generator=gen, device=dev) * 40 - 15).clamp_min(0).to(torch.int32)
        s = [[torch.zeros((n, 1), device=dev), torch.zeros((n, 1), device=dev), torch.zeros((n,), device=dev)] for _ in range(2)]
        tm = alternate({"hip": lambda: go.add_densification_stats(s[0][0], s[0][1], s[0][2], vgrad, radii),
                        "torch": lambda: torch_stats(s[1][0], s[1][1], s[1][2], vgrad, radii)}, a.warmup, a.reps, a.inner)
        same = torch.equal(s[0][1], s[1][1]) and torch.equal(s[0][2], s[1][2])
        lines.append(f"densification statistics, {n} Gaussians ({int((radii > 0).sum())} visible):  one launch {fmt(tm['hip'])}   three masked torch lines "
                     f"{fmt(tm['torch'])}   ratio {statistics.median(tm['torch']) / statistics.median(tm['hip']):.1f}   denom and max_radii2D equal: {same}")


def torch_densify(p, m, v, accum, denom, max_screen_size, z):
    """gaussian_model.py:353-405 on plain tensors: clone (cat), split (cat, prune of the parents), final prune"""
    def cat(new):
        for f in go.FIELDS:
            p[f] = torch.cat((p[f], new[f]), dim=0)
            m[f] = torch.cat((m[f], torch.zeros_like(new[f])), dim=0)
            v[f] = torch.cat((v[f], torch.zeros_like(new[f])), dim=0)

    def prune(mask):
        keep = ~mask
        for f in go.FIELDS:
            p[f], m[f], v[f] = p[f][keep], m[f][keep], v[f][keep]

    grads = accum / denom
    grads[grads.isnan()] = 0.0
    n0 = p["xyz"].shape[0]
    sel = (torch.norm(grads, dim=-1) >= MAX_GRAD) & (torch.exp(p["scaling"]).max(dim=1).values <= PERCENT_DENSE * EXTENT)
    cat({f: p[f][sel] for f in go.FIELDS})
    n1 = p["xyz"].shape[0]
    padded = torch.zeros((n1,), device=accum.device)
    padded[:n0] = grads.squeeze()
    sel = (padded >= MAX_GRAD) & (torch.exp(p["scaling"]).max(dim=1).values > PERCENT_DENSE * EXTENT)
    stds = torch.exp(p["scaling"][sel]).repeat(2, 1)
    samples = stds * z[:stds.shape[0]]
    q = torch.nn.functional.normalize(p["rotation"][sel])
    w, x, y, zz = q.unbind(1)
    rots = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y), 2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz),
                        2 * (y * zz - w * x), 2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3).repeat(2, 1, 1)
    new = {f: p[f][sel].repeat(2, *([1] * (p[f].dim() - 1))) for f in go.FIELDS}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + new["xyz"]
    new["scaling"] = torch.log(stds / 1.6)
    cat(new)
    prune(torch.cat((sel, torch.zeros(2 * int(sel.sum()), device=sel.device, dtype=torch.bool))))
    mask = (torch.sigmoid(p["opacity"]) < MIN_OPACITY).squeeze()
    if max_screen_size:
        mask = mask | (torch.exp(p["scaling"]).max(dim=1).values > 0.1 * EXTENT)
    prune(mask)
    m_rows = p["xyz"].shape[0]
    return torch.zeros((m_rows, 1), device=mask.device), torch.zeros((m_rows, 1), device=mask.device), torch.zeros((m_rows,), device=mask.device)


def densify_rows(a, dev, lines):
    for n in (100_000, 350_000):
        base = population(n, dev, seed=2, scales=(5e-3, 0.15))       # on both sides of percent_dense * extent = 0.05
        gen = torch.Generator(device=dev).manual_seed(n)
        mom = {f: torch.randn(base[f].shape, generator=gen, device=dev) * 1e-3 for f in go.FIELDS}
        sq = {f: torch.rand(base[f].shape, generator=gen, device=dev) * 1e-6 for f in go.FIELDS}
        denom = torch.randint(0, 4, (n, 1), generator=gen, device=dev).float()
        accum = torch.rand((n, 1), generator=gen, device=dev) * 4e-4 * denom
        z = torch.randn((2 * n, 3), generator=gen, device=dev)
        times = {"hip": [], "torch": []}
        rows = {}
        for rep in range(a.warmup + a.reps):
            for key in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if key == "hip":
                    res = go.densify_and_prune_tensors(base, mom, sq, accum, denom, MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, 20, noise=None, generator=gen)
                    rows[key] = (res.n_kept + res.n_cloned + res.n_split_children, res.n_split)
                else:
                    p, m, v = dict(base), dict(mom), dict(sq)
                    torch_densify(p, m, v, accum, denom, 20, z)
                    rows[key] = (p["xyz"].shape[0], None)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[key].append((time.perf_counter() - t0) * 1e3)
        lines.append(f"densify_and_prune, {n} Gaussians -> {rows['hip'][0]} rows ({rows['hip'][1]} split; torch restatement -> {rows['torch'][0]} rows), wall "
                     f"time with synchronises, noise drawn inside:  plan + emit {fmt(times['hip'])}   torch ops {fmt(times['torch'])}   ratio "
                     f"{statistics.median(times['torch']) / statistics.median(times['hip']):.1f}")


def iteration_rows(a, dev, lines):
    n, size = a.gaussians, 800
    cam = look_at_camera((0.0, -2.4, 0.3), (0.0, 0.0, 0.0), 40.0, size, size, up=(0.0, 0.0, -1.0))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    st = GaussianRasterizationSettings(size, size, cam["tanfovx"], cam["tanfovy"], t(np.ones(3, np.float32)), 1.0, t(cam["V"]), t(cam["P"]), 3,
                                       t(cam["campos"]), False, False)
    r = GaussianRasterizer(st)
    base = population(n, dev, seed=4)

    def render(by_name, means2D):
        shs = torch.cat((by_name["f_dc"], by_name["f_rest"]), dim=1)
        return r(means3D=by_name["xyz"], means2D=means2D, opacities=torch.sigmoid(by_name["opacity"]), shs=shs, scales=torch.exp(by_name["scaling"]),
                 rotations=torch.nn.functional.normalize(by_name["rotation"]))

    with torch.no_grad():
        target = render(base, None)[0]
        target = (target + 0.05 * torch.rand_like(target)).clamp(0, 1)

    def make(opt_cls, native_stats, **kw):
        opt = opt_cls(groups(base), lr=0.0, eps=1e-15, **kw)
        by_name = {g["name"]: g["params"][0] for g in opt.param_groups}
        stats = [torch.zeros((n, 1), device=dev), torch.zeros((n, 1), device=dev), torch.zeros((n,), device=dev)]

        def iteration():
            means2D = torch.zeros_like(by_name["xyz"], requires_grad=True)
            img, radii = render(by_name, means2D)
            photometric_loss(img, target).backward()
            with torch.no_grad():
                (go.add_densification_stats if native_stats else torch_stats)(stats[0], stats[1], stats[2], means2D.grad, radii)
                opt.step()
                opt.zero_grad(set_to_none=True)
        return iteration

    fns = {"native": make(go.GaussianAdam, True), "torch": make(torch.optim.Adam, False)}
    tm = alternate(fns, a.warmup, a.reps, max(a.inner // 4, 1))
    lines.append(f"one iteration (render {n} Gaussians with degree-3 shs at {size} x {size}, fused loss, backward, statistics, step):  native statistics + "
                 f"GaussianAdam {fmt(tm['native'])}   masked torch lines + torch.optim.Adam {fmt(tm['torch'])}   ratio "
                 f"{statistics.median(tm['torch']) / statistics.median(tm['native']):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_optim_table.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=100_000)
    ap.add_argument("--skip", nargs="*", default=[], choices=["adam", "stats", "densify", "iteration"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_optim_bench.py needs a HIP device: a CPU run gives no time")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/train_optim_bench.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} on {torch.cuda.get_device_name(0)}",
             "# median over the samples (min .. max); each sample is HIP events around back-to-back iterations (densify: wall time of one call); candidates alternate"]
    for name, fn in (("adam", adam_rows), ("stats", stats_rows), ("densify", densify_rows), ("iteration", iteration_rows)):
        if name in a.skip:
            lines.append(f"{name}: not measured in this run (--skip)")
            continue
        fn(a, dev, lines)
        print(lines[-1], flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
