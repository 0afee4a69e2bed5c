#!/usr/bin/env python
"""Pins the rasteriser's bits: SHA-256 digests of what GaussianRasterizer, FrameBatchRasterizer and the autograd backward write for a
fixed set of tests/_raster_ref.py scenes, and the values of the three *_workspace_bytes functions over a grid of arguments.

    python tests/golden/make_raster_bits.py --commit <the commit the library was built from>

writes tests/golden/raster_bits.json on a machine with an MI355X; tests/test_raster_bits_hip.py recomputes `CASES` with the tree
under test and compares for equality.  Uses only pixie_amd's Python API and tests/_raster_ref.py, so it runs on any commit that has
them.  The workspace sizes contain hipcub's temporary-storage needs, so the file holds for the ROCm version it records.

Cases (`CASES`): single forwards with aux=True -- scenes b, d, e, g, h, i through scales / rotations, scene a through both covariance
routes and with SHs of degree 3; batches of three views of scene i (view v sees pos * (1 + 0.02 v); the last 300 Gaussians are the
static tail) with SHs of degree 3 and with per-view colours, at a capacity of the largest view's count so that there are at least two
sort groups, and once, without a static tail, with the middle view behind scene f's camera where scene f's own cloud lies (its
Gaussians moved by z - 8: that view sees nothing); backwards with every gradient for scene d (cov3D, colors_precomp) and scene i (scales / rotations, SHs of degree 2)
under a fixed dL/dcolour."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from tests import _raster_ref as rr  # noqa: E402

PATH = os.path.join(REPO, "tests", "golden", "raster_bits.json")
STATIC_TAIL = 300


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def tens(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def settings_of(s, dev, sh_degree=0, cam=None):
    from pixie_amd.rasterizer import GaussianRasterizationSettings
    cam = cam or s["cam"]
    return GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                         bg=tens(s["bg"], dev), scale_modifier=s["scale_modifier"], viewmatrix=tens(cam["V"], dev),
                                         projmatrix=tens(cam["P"], dev), sh_degree=sh_degree, campos=tens(cam["campos"], dev), prefiltered=False,
                                         debug=False)


def cov_of(s):
    return rr.cov3d_from_scale_rot(s["scales"], s["rotations"], s["scale_modifier"], np.float32).reshape(-1, 6)


def shs_of(n, seed):
    return np.random.default_rng(seed).normal(0.0, 0.4, (n, 16, 3)).astype(np.float32)


def single(dev, name, route="sr", sh_degree=None):
    from pixie_amd.rasterizer import GaussianRasterizer
    s = rr.scene(name)
    n = len(s["means"])
    kw = dict(cov3D_precomp=tens(cov_of(s), dev)) if route == "cov" else dict(scales=tens(s["scales"], dev), rotations=tens(s["rotations"], dev))
    if sh_degree is None:
        kw["colors_precomp"] = tens(s["colors"].reshape(n, 3), dev)
    else:
        kw["shs"] = tens(shs_of(n, 77), dev)
    r = GaussianRasterizer(settings_of(s, dev, sh_degree or 0))
    with torch.no_grad():
        color, radii, final_T, n_contrib = r(tens(s["means"].reshape(n, 3), dev), None, tens(s["opacity"], dev), aux=True, **kw)
    return dict(color=digest(color), radii=digest(radii), final_T=digest(final_T), n_contrib=digest(n_contrib), last_instances=int(r.last_instances))


def batch(dev, colours, middle_away=False):
    from pixie_amd.rasterizer import FrameBatchRasterizer
    s, f = rr.scene("i"), rr.scene("f")
    n, views = len(s["means"]), 3
    means = np.stack([s["means"] * np.float32(1.0 + 0.02 * v) for v in range(views)]).astype(np.float32)
    settings = [settings_of(s, dev, 3)] * views
    if middle_away:
        means[1] += np.array([0.0, 0.0, -8.0], np.float32)      # behind the camera at z = -3, as scene f's own cloud is
        settings = [settings[0], settings_of(s, dev, 3, cam=f["cam"]), settings[0]]
    cov = cov_of(s)
    dyn = n if middle_away else n - STATIC_TAIL         # a static tail would stay in front of the middle view's camera
    args = (tens(means[:, :dyn], dev), tens(np.stack([cov[:dyn]] * views), dev), settings, tens(s["opacity"], dev))
    if colours == "shs":
        kw = dict(shs=tens(shs_of(n, 78), dev))
    else:
        kw = dict(colors_precomp=tens(np.random.default_rng(79).uniform(0.0, 1.0, (views, n, 3)).astype(np.float32), dev))
    if dyn < n:
        kw["static"] = (tens(s["means"][dyn:], dev), tens(cov[dyn:], dev))
    r = FrameBatchRasterizer()
    r(*args, **kw)                                       # the per-view counts
    capacity = max(r.last_instances)
    got = r(*args, out=True, out_rgb8=True, aux=True, capacity=capacity, **kw)
    assert r.last_groups >= 2, "the forced capacity must split the views into at least two sort groups"
    assert not middle_away or r.last_instances[1] == 0, "the middle view must see nothing"
    return dict(color=digest(got.color), rgb8=digest(got.rgb8), radii=digest(got.radii), final_T=digest(got.final_T),
                n_contrib=digest(got.n_contrib), last_instances=[int(c) for c in r.last_instances], last_groups=int(r.last_groups),
                capacity=int(capacity))


def backward(dev, name, route, sh_degree, g):
    from pixie_amd.rasterizer import GaussianRasterizer
    s = rr.scene(name)
    n = len(s["means"])
    x = dict(means3D=tens(s["means"].reshape(n, 3), dev), opacities=tens(s["opacity"].reshape(n, 1), dev))
    x["means2D"] = torch.zeros_like(x["means3D"])
    if route == "cov":
        x["cov3D_precomp"] = tens(cov_of(s), dev)
    else:
        x["scales"], x["rotations"] = tens(s["scales"], dev), tens(s["rotations"], dev)
    if sh_degree is None:
        x["colors_precomp"] = tens(s["colors"].reshape(n, 3), dev)
    else:
        x["shs"] = tens(shs_of(n, 80), dev)
    for t in x.values():
        t.requires_grad_(True)
    r = GaussianRasterizer(settings_of(s, dev, sh_degree or 0))
    color, radii = r(x["means3D"], x["means2D"], x["opacities"], **{k: v for k, v in x.items() if k not in ("means3D", "means2D", "opacities")})
    color.backward(tens(g, dev))
    out = dict(color=digest(color), radii=digest(radii), last_instances=int(r.last_instances))
    for k, t in x.items():
        assert t.grad is not None, k
        out["grad_" + k] = digest(t.grad)
    return out


def backward_cases(dev):
    rng = np.random.default_rng(5)                       # one stream: scene d's dL/dcolour, then scene i's
    out = {}
    for tag, name, route, degree in (("backward d cov3D colors", "d", "cov", None), ("backward i scales/rotations shs2", "i", "sr", 2)):
        cam = rr.scene(name)["cam"]
        out[tag] = backward(dev, name, route, degree, rng.uniform(-1.0, 1.0, (3, cam["H"], cam["W"])).astype(np.float32))
    return out


def workspace_sizes(dev):
    from pixie_amd import _lib
    lib = _lib.load()
    out = {}
    with torch.cuda.device(dev):
        for n in (0, 1, 255, 256, 257, 5000):
            for W, H in ((16, 16), (17, 33), (800, 800)):
                for m in sorted({0, 1, 4 * n}):
                    key = f"n {n} image {W}x{H} instances {m}"
                    out[key + " forward"] = int(lib.pixie_raster_workspace_bytes(n, W, H, m))
                    out[key + " backward"] = int(lib.pixie_raster_backward_workspace_bytes(n, W, H, m))
                    for views in (1, 3):
                        out[key + f" batch of {views}"] = int(lib.pixie_raster_batch_workspace_bytes(n, views, W, H, m))
    return out


CASES = {f"single {name}": (lambda dev, name=name: single(dev, name)) for name in ("b", "d", "e", "g", "h", "i")}
CASES["single a cov3D"] = lambda dev: single(dev, "a", route="cov")
CASES["single a scales/rotations"] = lambda dev: single(dev, "a")
CASES["single a shs3"] = lambda dev: single(dev, "a", sh_degree=3)
CASES["batch i shs3"] = lambda dev: batch(dev, "shs")
CASES["batch i per-view colors"] = lambda dev: batch(dev, "colors")
CASES["batch i middle view sees nothing"] = lambda dev: batch(dev, "colors", middle_away=True)
CASES["backward"] = backward_cases
CASES["workspace bytes"] = workspace_sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under pixie_amd/ was built from")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = dict(commit=a.commit, rocm=str(torch.version.hip), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               cases={name: fn(dev) for name, fn in CASES.items()})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(doc['cases'])} cases")


if __name__ == "__main__":
    main()
