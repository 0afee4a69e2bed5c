#!/usr/bin/env python
"""Times the two training natives -- the fused photometric loss (pixie_amd/losses.py) and distCUDA2 (pixie_amd/simple_knn.py) --
against the same computations written as torch ops on the same device, and one whole 3DGS training iteration (differentiable
render + loss + backward) with either loss.  Writes a table (default profiles/train_natives_table.txt); recorded, not asserted.

Method: every pair (ours, torch) alternates in the same process, `--warmup` rounds of both first; each sample is HIP events around
`--inner` back-to-back iterations; the table gives the median over `--reps` samples and the spread (min .. max).
  * loss rows: forward + backward of (1 - 0.2) L1 + 0.2 (1 - SSIM) with respect to the image, at 800 x 800 x 3 and 64 x 64 x 3.  The
    torch side is the reference's expression (five grouped 11 x 11 conv2d and the elementwise ops, autograd backward).
  * iteration rows: GaussianRasterizer at `--gaussians` Gaussians, 800 x 800, means / opacities / colours / covariances requiring
    grad, then either loss, then backward through both.
  * distCUDA2 rows: 100 k and 1 M uniform points and a clustered cloud (half N(100, 1e-3), half N(0, 5), 100 k), against a chunked
    torch.cdist + topk(4, smallest).  At 1 M the torch side is timed on `--cdist-chunks` chunks of 1024 query rows and scaled to all
    rows, which the row says.
"""
import argparse
import os
import statistics
import sys
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pixie_amd.losses import photometric_loss  # noqa: E402
from pixie_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from pixie_amd.simple_knn import distCUDA2  # noqa: E402
from scripts.raster_bench import look_at_camera  # noqa: E402


def torch_window(channels, dev):
    g = torch.tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    w = (g / g.sum()).unsqueeze(1)
    return w.mm(w.t()).float().unsqueeze(0).unsqueeze(0).expand(channels, 1, 11, 11).contiguous().to(dev)


def torch_loss(img, gt, window, lam=0.2):
    """utils/loss_utils.py l1_loss and ssim and the combination of train.py:92, the window built once outside"""
    c = img.shape[-3]
    a, b = (img[None], gt[None]) if img.dim() == 3 else (img, gt)
    mu1, mu2 = F.conv2d(a, window, padding=5, groups=c), F.conv2d(b, window, padding=5, groups=c)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(a * a, window, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(b * b, window, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(a * b, window, padding=5, groups=c) - mu12
    ssim_map = ((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return (1.0 - lam) * torch.abs(img - gt).mean() + lam * (1.0 - ssim_map.mean())


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fns, warmup, reps, inner):
    """{name: [ms per iteration] * reps}, the candidates taking turns"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(sample(fn, inner))
    return times


def fmt(ts):
    return f"{statistics.median(ts):9.4f} ms  ({min(ts):.4f} .. {max(ts):.4f})"


def loss_rows(a, dev, lines):
    for size in (800, 64):
        gen = torch.Generator(device="cpu").manual_seed(size)
        img = torch.rand((3, size, size), generator=gen).to(dev).requires_grad_(True)
        gt = torch.rand((3, size, size), generator=gen).to(dev)
        window = torch_window(3, dev)

        def fused():
            img.grad = None
            photometric_loss(img, gt).backward()

        def expr():
            img.grad = None
            torch_loss(img, gt, window).backward()

        t = alternate(dict(fused=fused, torch=expr), a.warmup, a.reps, a.inner)
        fused(); g1 = img.grad.clone(); expr(); g2 = img.grad.clone()
        rel = float(torch.linalg.norm((g1 - g2).double()) / torch.linalg.norm(g2.double()))
        lines.append(f"loss forward + backward, {size} x {size} x 3:  fused {fmt(t['fused'])}   torch expression {fmt(t['torch'])}   "
                     f"ratio {statistics.median(t['torch']) / statistics.median(t['fused']):.2f}   gradients differ by {rel:.1e} rel-L2")


def iteration_rows(a, dev, lines):
    n, size = a.gaussians, 800
    rng = np.random.default_rng(0)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (d * (0.5 * rng.random(n) ** (1 / 3))[:, None]).astype(np.float32)
    s2 = rng.uniform(1e-5, 4e-5, n).astype(np.float32)
    cov = np.zeros((n, 6), np.float32)
    cov[:, 0] = cov[:, 3] = cov[:, 5] = s2
    cam = look_at_camera((0.0, -2.4, 0.3), (0.0, 0.0, 0.0), 40.0, size, size, up=(0.0, 0.0, -1.0))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    st = GaussianRasterizationSettings(size, size, cam["tanfovx"], cam["tanfovy"], t(np.ones(3, np.float32)), 1.0, t(cam["V"]), t(cam["P"]), 0,
                                       t(cam["campos"]), False, False)
    r = GaussianRasterizer(st)
    leaves = dict(means3D=t(pos), opacities=t(rng.uniform(0.2, 1.0, (n, 1)).astype(np.float32)),
                  colors_precomp=t(rng.uniform(0, 1, (n, 3)).astype(np.float32)), cov3D_precomp=t(cov))
    with torch.no_grad():
        target = r(means2D=None, **leaves)[0]
        target = (target + 0.05 * torch.rand_like(target)).clamp(0, 1)
    params = [v.requires_grad_(True) for v in leaves.values()]
    means2D = torch.zeros_like(leaves["means3D"])
    window = torch_window(3, dev)

    def step(loss_fn):
        for p in params:
            p.grad = None
        img = r(means2D=means2D, **leaves)[0]
        loss_fn(img).backward()

    fns = dict(fused=lambda: step(lambda img: photometric_loss(img, target)), torch=lambda: step(lambda img: torch_loss(img, target, window)),
               render_only=lambda: step(lambda img: img.sum()))
    tm = alternate(fns, a.warmup, a.reps, max(a.inner // 2, 1))
    lines.append(f"one iteration (render {n} Gaussians at {size} x {size} + loss + backward):  fused loss {fmt(tm['fused'])}   "
                 f"torch loss {fmt(tm['torch'])}   render + backward of sum() alone {fmt(tm['render_only'])}")


def cdist_knn(p, chunk=1024, max_chunks=None):
    """mean squared distance to the three nearest others by chunked cdist + topk; returns (values, rows done)"""
    n = p.shape[0]
    out = torch.empty((n,), dtype=torch.float32, device=p.device)
    done = 0
    for k, s in enumerate(range(0, n, chunk)):
        if max_chunks is not None and k >= max_chunks:
            break
        d = torch.cdist(p[s:s + chunk], p)
        best = torch.topk(d, 4, dim=1, largest=False).values[:, 1:]
        out[s:s + chunk] = (best * best).sum(dim=1) / 3.0
        done = min(n, s + chunk)
    return out, done


def knn_rows(a, dev, lines):
    rng = np.random.default_rng(1)
    clouds = [("100 k uniform", rng.uniform(-1, 1, (100_000, 3)), None), ("1 M uniform", rng.uniform(-1, 1, (1_000_000, 3)), a.cdist_chunks),
              ("100 k clustered", np.concatenate([rng.normal(100.0, 1e-3, (50_000, 3)), rng.normal(0.0, 5.0, (50_000, 3))]), None)]
    for name, pts, max_chunks in clouds:
        p = torch.from_numpy(pts.astype(np.float32)).to(dev)
        n = p.shape[0]
        ours = alternate(dict(knn=lambda: distCUDA2(p)), a.warmup, a.reps, 2)["knn"]
        base = []
        for rep in range(1 + min(a.reps, 3)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ref, done = cdist_knn(p, max_chunks=max_chunks)
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:                                # the first is the warm-up
                base.append(e0.elapsed_time(e1) * n / done)
        got = distCUDA2(p)
        rel = float(((got[:done] - ref[:done]).abs() / ref[:done].clamp_min(1e-30)).median())
        note = "" if done == n else f" (timed on {done} of {n} query rows and scaled)"
        lines.append(f"distCUDA2, {name}:  HIP {fmt(ours)}   chunked cdist + topk {fmt(base)}{note}   ratio "
                     f"{statistics.median(base) / statistics.median(ours):.1f}   median relative difference of the values {rel:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_natives_table.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=100_000)
    ap.add_argument("--cdist-chunks", type=int, default=16)
    ap.add_argument("--skip", nargs="*", default=[], choices=["loss", "iteration", "knn"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench.py needs a HIP device: a CPU run gives no time")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/train_step_bench.py --reps {a.reps} --warmup {a.warmup} --inner {a.inner} on {torch.cuda.get_device_name(0)}",
             "# median over the samples (min .. max); each sample is HIP events around back-to-back iterations; candidates alternate"]
    for name, fn in (("loss", loss_rows), ("iteration", iteration_rows), ("knn", knn_rows)):
        if name not in a.skip:
            fn(a, dev, lines)
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
