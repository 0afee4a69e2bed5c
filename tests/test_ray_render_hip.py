"""GPU checks of the differentiable ray compositing (pixie_amd.ray_render, pixie_amd/csrc/ray_render.hip) against the torch restatement
of the reference's lines in tests/_ray_render_ref.py, whose gradients come from autograd.

Bar, for every output and gradient array: max |got - ref64| <= 3 x max |yard32 - ref64| + K 2^-24 max(1, max |ref64|), the yardstick
being the restatement in float32 on the CPU and K the number of terms of the longest sum behind the array plus 16: S for the ray sums
(and for d_rgb / d_features, which carry a weight or 1 - accumulation), S + C for d_density, whose g_i holds a C-term dot product.
The upstream gradients are fixed random arrays for every output at once.

Median depth, no exclusions: the value must be bit-equal to the float32 mid-point of an index j with cum64[j] >= 0.5 - tau and
(j == 0 or cum64[j - 1] < 0.5 + tau), tau = S 2^-23; a ray that never reaches 0.5 returns the last sample.

The measured ratios are appended to the file named by PIXIE_RAY_PARITY_OUT when it is set (profiles/ray_composite_parity.txt is such
a run's output).
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import _field_query_ref as R
from tests import _hashmlp_grad_ref as G
from tests import _ray_render_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_KEYS = ("densities", "rgb", "features")
TINT = (0.2, 0.5, 0.7)

# (R, S, C, background): S in {1, 2, 47, 48, 64, 65, 96, 256} with features, {1000, 1024} weights only; C in {4, 252, 256, 260, 768};
# R in {1, 3, 130}; each background mode
CASES = [(1, 1, 4, "last_sample"), (3, 2, 252, "random"), (130, 47, 4, "white"), (130, 48, 768, "last_sample"), (3, 64, 256, TINT),
         (3, 65, 260, "last_sample"), (130, 96, 252, "random"), (3, 256, 768, "white"), (1, 48, 768, "random"), (130, 1000, 0, "last_sample"),
         (3, 1024, 0, TINT)]


def note(line):
    print(line)
    path = os.environ.get("PIXIE_RAY_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def reference(n_rays, n_samples, n_channels, background, seed=0):
    """inputs, upstream gradients and the restatement in float64 and float32: computed once, shared, never modified"""
    inp = ref.make_inputs(n_rays, n_samples, n_channels, seed=seed + 17 * n_samples + n_channels)
    up = ref.make_upstream(n_rays, n_samples, n_channels, seed=seed + 1000 + n_samples)
    return inp, up, ref.evaluate(inp, up, torch.float64, background), ref.evaluate(inp, up, torch.float32, background)


def ours(inp, up, background, needs=GRAD_KEYS):
    from pixie_amd import ray_render
    t = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if v is not None else None) for k, v in inp.items()}
    for k in needs:
        if t[k] is not None:
            t[k].requires_grad_(True)
    out = ray_render.composite(t["densities"], t["deltas"], t["starts"], t["ends"], t["rgb"], t["features"], background)
    loss = None
    for k in ref.OUTPUTS:
        if out[k] is not None and up.get(k) is not None:
            term = (out[k] * torch.from_numpy(up[k]).to(DEV)).sum()
            loss = term if loss is None else loss + term
    if loss is not None and loss.requires_grad:
        loss.backward()
    host = lambda v: v.detach().cpu().numpy() if v is not None else None
    return {k: host(v) for k, v in out.items()}, {k: host(t[k].grad) for k in GRAD_KEYS if t[k] is not None and t[k].grad is not None}


def terms_of(name, n_samples, n_channels):
    return n_samples + n_channels if name == "d_densities" else n_samples


def within(what, name, got, r64, r32, terms):
    assert got is not None and got.shape == r64.shape and np.all(np.isfinite(got)), f"{what} {name}"
    err = float(np.max(np.abs(got.astype(np.float64) - r64), initial=0.0))
    yd = float(np.max(np.abs(r32 - r64), initial=0.0))
    limit = ref.bar(r64, r32, terms)
    note(f"{what} {name}: max|got - f64| {err:.3e}, float32 CPU {yd:.3e} (ratio {err / yd if yd else float('inf'):.2f}), bar {limit:.3e}")
    assert err <= limit, f"{what} {name}: {err:.3e} > {limit:.3e}"


def compare(what, got, want64, want32, n_samples, n_channels):
    (o, g), (o64, g64), (o32, g32) = got, want64, want32
    for k in ref.OUTPUTS:
        if o64[k] is None:
            assert o[k] is None, k
            continue
        within(what, k, o[k], o64[k], o32[k], terms_of(k, n_samples, n_channels))
    assert set(g) == set(g64), (set(g), set(g64))
    for k in g64:
        within(what, "d_" + k, g[k], g64[k], g32[k], terms_of("d_" + k, n_samples, n_channels))


# ---- 1. every output and gradient against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"R{c[0]}_S{c[1]}_C{c[2]}_{c[3] if isinstance(c[3], str) else 'tint'}")
def test_outputs_and_gradients_against_float64(case):
    n_rays, n_samples, n_channels, background = case
    inp, up, want64, want32 = reference(*case)
    got = ours(inp, up, background)
    compare(f"({n_rays}, {n_samples}, {n_channels}) {background}", got, want64, want32, n_samples, n_channels)
    ok = ref.median_admissible(got[0]["depth"], want64[0]["weights"], inp["starts"], inp["ends"], n_samples)
    assert ok.all(), f"median depth of rays {np.nonzero(~ok)[0][:8]} is no admissible mid-point"
    acc = want64[0]["accumulation"]
    if n_rays == 130:
        assert acc.min() < 0.1 and acc.max() > 0.999, "the inputs must hold near-empty and saturated rays"


# ---- 2. every subset of present inputs and wanted gradients ------------------------------------------------------------------------
SUBSETS = [dict(drop=("rgb", "features")), dict(drop=("rgb",)), dict(drop=("features",)), dict(needs=("densities",)), dict(needs=("rgb",)),
           dict(needs=("features",)), dict(needs=("rgb", "features")), dict(only=("feature",)), dict(only=("weights",)), dict(only=("rgb",)),
           dict(only=("accumulation", "expected_depth")), dict(only=("rgb",), needs=("rgb",)), dict(only=("feature",), needs=("features",))]


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "-".join(f"{k}_{'+'.join(v)}" for k, v in s.items()))
def test_absent_inputs_and_unwanted_gradients(subset):
    n_rays, n_samples, n_channels = 5, 47, 8
    inp, up, _, _ = reference(n_rays, n_samples, n_channels, "last_sample")
    inp = {k: (None if k in subset.get("drop", ()) else v) for k, v in inp.items()}
    up = {k: (v if k in subset.get("only", ref.OUTPUTS) else None) for k, v in up.items()}
    needs = subset.get("needs", GRAD_KEYS)
    o, g = ours(inp, up, "last_sample", needs)
    want64, want32 = (ref.evaluate(inp, up, d, "last_sample") for d in (torch.float64, torch.float32))
    # autograd gives the restatement a zero gradient where ours reports none: an input that reaches no output with an upstream gradient
    reach = {"densities": True, "rgb": up["rgb"] is not None, "features": up["feature"] is not None}
    keep = [k for k in needs if inp[k] is not None and reach[k]]
    assert sorted(g) == sorted(keep), (sorted(g), keep)
    trim = lambda e: (e[0], {k: v for k, v in e[1].items() if k in keep})
    compare(f"subset {subset}", (o, g), trim(want64), trim(want32), n_samples, n_channels)


# ---- 3. special rays ---------------------------------------------------------------------------------------------------------------
def test_special_rays():
    n_rays, n_samples, n_channels, nan_at, inf_at = 8, 24, 8, 10, 5
    base, up, _, _ = reference(n_rays, n_samples, n_channels, "last_sample", seed=5)
    inp = {k: v.copy() for k, v in base.items()}
    inp["densities"][0] = 0.0                                              # empty ray
    inp["densities"][1, 0] = np.float32(1e4) / inp["deltas"][1, 0]         # delta sigma = 1e4 on the first sample
    inp["deltas"][2] = 0.0                                                 # delta = 0 everywhere
    inp["densities"][3, nan_at] = np.nan
    inp["densities"][4, inf_at] = np.inf
    with np.errstate(all="ignore"):
        (o64, _), (o32, _) = ref.evaluate(inp, {}, torch.float64), ref.evaluate(inp, {}, torch.float32)
    o, g = ours(inp, up, "last_sample")
    for k in ref.OUTPUTS:
        within("special rays", k, o[k], o64[k], o32[k], n_samples)
    assert ref.median_admissible(o["depth"], o64["weights"], inp["starts"], inp["ends"], n_samples).all()
    steps = ((inp["starts"] + inp["ends"]) / np.float32(2)).astype(np.float32)
    assert np.all(o["weights"][0] == 0) and o["accumulation"][0] == 0 and o["expected_depth"][0, 0] == steps.min()
    assert np.array_equal(o["rgb"][0], inp["rgb"][0, -1]) and o["depth"][0, 0] == steps[0, -1, 0] and np.all(o["feature"][0] == 0)
    assert o["weights"][1, 0, 0] == 1.0 and np.all(o["weights"][1, 1:] == 0) and o["depth"][1, 0] == steps[1, 0, 0]
    assert np.all(o["weights"][2] == 0) and o["accumulation"][2] == 0
    assert np.all(o["weights"][3, :nan_at] > 0) and np.all(o["weights"][3, nan_at:] == 0)
    assert np.array_equal(o["weights"][3, :nan_at], ours(base, {}, "last_sample")[0]["weights"][3, :nan_at]), "weights before the NaN are as usual"
    assert o["weights"][4, inf_at, 0] > 0 and np.all(o["weights"][4, inf_at + 1:] == 0)
    # the NaN ray: every gradient finite, zero on the masked samples (rgb's last sample carries the background's (1 - acc) dRGB)
    for k in GRAD_KEYS:
        assert np.all(np.isfinite(g[k][3])), k
    assert np.all(g["densities"][3, nan_at:] == 0) and np.all(g["features"][3, nan_at:] == 0) and np.all(g["rgb"][3, nan_at:-1] == 0)
    # before the NaN: the restatement's gradient on the masked weights (NaN taken out of the densities, weights times keep)
    clean = {k: v.copy() for k, v in inp.items()}
    clean["densities"][3, nan_at] = 1.0
    clean["densities"][4, inf_at] = 1.0                                    # torch's own NaN gradients on that ray are not the subject
    keep = np.ones((n_rays, n_samples, 1))
    keep[3, nan_at:] = 0
    (_, g64), (_, g32) = (ref.evaluate(clean, up, d, "last_sample", keep=keep) for d in (torch.float64, torch.float32))
    for k in GRAD_KEYS:
        sel = (3, slice(0, nan_at)) if k == "densities" else 3
        within("NaN ray", "d_" + k, g[k][sel], g64[k][sel], g32[k][sel], terms_of("d_" + k, n_samples, n_channels))
    for k in GRAD_KEYS:                                                     # and the untouched rays are untouched
        within("special rays, plain rays", "d_" + k, g[k][5:], g64[k][5:], g32[k][5:], terms_of("d_" + k, n_samples, n_channels))
    assert np.all(np.isfinite(g["densities"][4])), "an Inf density leaves finite gradients"


# ---- 4. structure ------------------------------------------------------------------------------------------------------------------
def split_calls(inp, up, background):
    """the reference's call sequence (f3rm/model.py:206-222) on get_weights and the four renderer classes"""
    from pixie_amd import ray_render
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in inp.items()}
    for k in GRAD_KEYS:
        t[k].requires_grad_(True)
    samples = types.SimpleNamespace(frustums=types.SimpleNamespace(starts=t["starts"], ends=t["ends"]))
    weights = ray_render.get_weights(t["densities"], t["deltas"])
    out = {"weights": weights, "rgb": ray_render.RGBRenderer(background).train()(rgb=t["rgb"], weights=weights)}
    with torch.no_grad():
        out["depth"] = ray_render.DepthRenderer("median")(weights=weights, ray_samples=samples)
    out["expected_depth"] = ray_render.DepthRenderer("expected")(weights=weights, ray_samples=samples)
    out["accumulation"] = ray_render.AccumulationRenderer()(weights=weights)
    out["feature"] = ray_render.FeatureRenderer()(features=t["features"], weights=weights)
    loss = None
    for k in ref.OUTPUTS:
        term = (out[k] * torch.from_numpy(up[k]).to(DEV)).sum()
        loss = term if loss is None else loss + term
    loss.backward()
    host = lambda v: v.detach().cpu().numpy()
    return {k: host(v) for k, v in out.items()}, {k: host(t[k].grad) for k in GRAD_KEYS}


def same_bits(a, b, what):
    for part_a, part_b in zip(a, b):
        assert part_a.keys() == part_b.keys(), what
        for k in part_a:
            assert np.array_equal(part_a[k].view(np.uint32), part_b[k].view(np.uint32)), f"{what}: {k} differs"


@pytest.mark.parametrize("background", ["last_sample", "random", TINT], ids=["last_sample", "random", "tint"])
def test_composite_equals_the_split_calls_bit_for_bit(background):
    inp, up, _, _ = reference(130, 48, 260, "last_sample", seed=3)
    same_bits(ours(inp, up, background), split_calls(inp, up, background), "composite vs get_weights + renderers")


def test_runs_permutations_and_batch_size_leave_the_bits():
    n_rays = 130
    inp, up, _, _ = reference(n_rays, 65, 260, "last_sample", seed=4)
    first = ours(inp, up, "last_sample")
    same_bits(first, ours(inp, up, "last_sample"), "two runs")
    perm = np.random.default_rng(0).permutation(n_rays)
    moved = ours({k: v[perm] for k, v in inp.items()}, {k: v[perm] for k, v in up.items()}, "last_sample")
    same_bits(tuple({k: v[perm] for k, v in part.items()} for part in first), moved, "permuted rays")
    j = 77
    alone = ours({k: v[j:j + 1] for k, v in inp.items()}, {k: v[j:j + 1] for k, v in up.items()}, "last_sample")
    steps = (inp["starts"][j] + inp["ends"][j]) / 2
    assert steps.min() < first[0]["expected_depth"][j] < steps.max(), "pick a ray that its own range does not clip"
    same_bits(tuple({k: v[j:j + 1] for k, v in part.items()} for part in first), alone, "R = 1 against the same ray inside R = 130")


def test_eval_mode_rgb_renderer_and_leading_dimensions():
    from pixie_amd import ray_render
    inp, _, _, _ = reference(6, 47, 0, "last_sample", seed=6)
    rgb = (inp["rgb"] * 6 - 2.5).astype(np.float32)
    rgb[2, 5, 1] = np.nan
    shape = lambda a: torch.from_numpy(a).to(DEV).reshape(2, 3, *a.shape[1:])
    weights = ray_render.get_weights(shape(inp["densities"]), shape(inp["deltas"]))
    assert weights.shape == (2, 3, 47, 1)
    got = ray_render.RGBRenderer("white").eval()(rgb=shape(rgb), weights=weights)
    assert got.shape == (2, 3, 3)
    w64 = ref.get_weights(torch.tensor(inp["densities"], dtype=torch.float64), torch.tensor(inp["deltas"], dtype=torch.float64))
    want = torch.clamp(ref.combine_rgb(torch.nan_to_num(torch.tensor(rgb, dtype=torch.float64)), w64, "white"), 0.0, 1.0).numpy()
    assert np.max(np.abs(got.cpu().numpy().reshape(6, 3) - want)) <= (47 + 16) * 2.0 ** -24 * 3.5 and got.min() >= 0 and got.max() <= 1
    assert (want == 0).any() and (want == 1).any(), "the clamp must bite on both sides"


# ---- 5. the tail of get_outputs / get_loss_dict on a trainable feature net ------------------------------------------------------------
def distortion_loss(weights, starts, ends):
    """nerfstudio's distortion_loss / lossfun_distortion (model_components/losses.py:135-154), torch's own ops"""
    t = torch.cat([starts[..., 0], ends[..., -1:, 0]], dim=-1) / 4.05
    w = weights[..., 0]
    ut = (t[..., 1:] + t[..., :-1]) / 2
    dut = torch.abs(ut[..., :, None] - ut[..., None, :])
    loss_inter = torch.sum(w * torch.sum(w[..., None, :] * dut, dim=-1), dim=-1)
    loss_intra = torch.sum(w ** 2 * (t[..., 1:] - t[..., :-1]), dim=-1) / 3
    return torch.mean(loss_inter + loss_intra)


def tail_loss(out, target_rgb, target_feature, starts, ends):
    mse = torch.nn.functional.mse_loss
    return mse(out["rgb"], target_rgb) + 1e-3 * mse(out["feature"], target_feature) + 0.002 * distortion_loss(out["weights"], starts, ends)


def integration_case():
    """a feature net without an undecided ReLU at its points (chosen from the float64 forward alone), rays, targets"""
    n_rays, n_samples, n_channels = 32, 16, 8
    for seed in range(50):
        rng = np.random.default_rng(300 + seed)
        lv, rows = R.levels("tcnn", 2, 8, 16, 10)
        net = R.random_net(rng, lv, rows, 2, n_hidden=1, out_dim=n_channels)
        p = rng.random((n_rays * n_samples, 3)).astype(np.float32)
        P = G.params(net, torch.float64)
        with torch.no_grad():
            _, zs, xs = G.forward(net, P, p, None)
        if not G.undecided(P, zs, xs).any():
            break
    else:
        raise AssertionError("no seed without an undecided ReLU")
    inp = ref.make_inputs(n_rays, n_samples, 0, seed=seed)
    targets = (rng.uniform(0, 1, (n_rays, 3)).astype(np.float32), rng.standard_normal((n_rays, n_channels)).astype(np.float32))
    return net, p, inp, targets, (n_rays, n_samples, n_channels)


def restated_tail(net, p, inp, targets, shape, dtype, steps=0):
    """gradients of the tail's loss (steps == 0) or the losses of `steps` Adam steps on the net's parameters and the rgb, on the CPU"""
    n_rays, n_samples, n_channels = shape
    P = G.params(net, dtype)
    leaves = [P["table"]] + P["weights"] + [b for b in P["biases"] if b is not None]
    t = {k: torch.tensor(v, dtype=dtype) for k, v in inp.items() if v is not None}
    t["densities"].requires_grad_(True), t["rgb"].requires_grad_(True)
    tr, tf = (torch.tensor(v, dtype=dtype) for v in targets)

    def loss_of():
        features = G.forward(net, P, p, None, dtype)[0].reshape(n_rays, n_samples, n_channels)
        return tail_loss(ref.get_outputs(t["densities"], t["deltas"], t["starts"], t["ends"], t["rgb"], features), tr, tf, t["starts"], t["ends"])

    if steps == 0:
        loss_of().backward()
        g = lambda v: None if v is None else v.grad.double().numpy()
        return dict(table=g(P["table"]), weights=[g(w) for w in P["weights"]], biases=[g(b) for b in P["biases"]],
                    densities=g(t["densities"]), rgb=g(t["rgb"]))
    opt = torch.optim.Adam(leaves + [t["rgb"]], lr=1e-2, eps=1e-15)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = loss_of()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return losses


def device_tail(net, p, inp, targets, shape):
    from pixie_amd import field_query as FQ, field_training as FT, ray_render
    n_rays, n_samples, n_channels = shape
    lv = np.array([tuple(l[k] for k in FQ.LEVEL_DTYPE.names) for l in net["levels"]], FQ.LEVEL_DTYPE)
    module = FT.TrainableHashMLP(lv, net["table"], net["weights"], net["biases"], net["n_frequencies"], net["n_extra"], net["act"], device=DEV)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items() if v is not None}
    t["densities"].requires_grad_(True), t["rgb"].requires_grad_(True)
    pos, (tr, tf) = torch.from_numpy(p).to(DEV), (torch.from_numpy(v).to(DEV) for v in targets)
    samples = types.SimpleNamespace(frustums=types.SimpleNamespace(starts=t["starts"], ends=t["ends"]))
    renderers = (ray_render.RGBRenderer("last_sample"), ray_render.DepthRenderer("median"), ray_render.DepthRenderer("expected"),
                 ray_render.AccumulationRenderer(), ray_render.FeatureRenderer())

    def loss_of():
        features = module(pos).reshape(n_rays, n_samples, n_channels)
        weights = ray_render.get_weights(t["densities"], t["deltas"])
        out = {"weights": weights, "rgb": renderers[0](rgb=t["rgb"], weights=weights)}
        with torch.no_grad():
            out["depth"] = renderers[1](weights=weights, ray_samples=samples)
        out["expected_depth"] = renderers[2](weights=weights, ray_samples=samples)
        out["accumulation"] = renderers[3](weights=weights)
        out["feature"] = renderers[4](features=features, weights=weights)
        return tail_loss(out, tr, tf, t["starts"], t["ends"])

    return module, t, loss_of


def test_get_outputs_tail_gradients_end_to_end():
    net, p, inp, targets, shape = integration_case()
    ref64, yard32 = (restated_tail(net, p, inp, targets, shape, d) for d in (torch.float64, torch.float32))
    module, t, loss_of = device_tail(net, p, inp, targets, shape)
    loss_of().backward()
    host = lambda v: None if v is None else v.grad.cpu().numpy()
    got = dict(table=host(module.table), weights=[host(w) for w in module.weights], biases=[host(b) for b in module.bias_list()])
    flat = lambda g: [("d_table", g["table"])] + [(f"d_weight[{i}]", w) for i, w in enumerate(g["weights"])] + \
        [(f"d_bias[{i}]", b) for i, b in enumerate(g["biases"])]
    for (name, a), (_, r), (_, y) in zip(flat(got), flat(ref64), flat(yard32)):
        err, limit = float(np.max(np.abs(a.astype(np.float64) - r))), float(G.bar(r, y, [net]))
        note(f"get_outputs tail {name}: max|got - f64| {err:.3e}, float32 CPU {float(np.max(np.abs(y - r))):.3e}, bar {limit:.3e}")
        assert np.all(np.isfinite(a)) and err <= limit, name
    for k in ("densities", "rgb"):
        within("get_outputs tail", "d_" + k, host(t[k]), ref64[k], yard32[k], shape[1] + shape[2])


def test_get_outputs_tail_trains():
    net, p, inp, targets, shape = integration_case()
    steps = 20
    losses = restated_tail(net, p, inp, targets, shape, torch.float32, steps)
    first, measure = losses[0], losses[-1]
    assert measure < first, f"the measure does not train: {first:.4e} -> {measure:.4e}"
    module, t, loss_of = device_tail(net, p, inp, targets, shape)
    opt = torch.optim.Adam(list(module.parameters()) + [t["rgb"]], lr=1e-2, eps=1e-15)
    for _ in range(steps):
        opt.zero_grad()
        loss_of().backward()
        opt.step()
    with torch.no_grad():
        final = float(loss_of())
    note(f"get_outputs tail trains: initial loss {first:.6e}; after {steps} Adam steps the float32 CPU restatement {measure:.6e}, ours {final:.6e}")
    assert final < first and final <= 2 * measure


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pixie_amd import _lib, ray_render
    dev = lambda *s: torch.rand(*s, device=DEV)
    d, f, c = dev(4, 8, 1), dev(4, 8, 8), dev(4, 8, 3)
    samples = types.SimpleNamespace(frustums=types.SimpleNamespace(starts=d, ends=d))
    assert ray_render.get_weights(d, d).shape == (4, 8, 1)
    with pytest.raises(ValueError):
        ray_render.get_weights(d.double(), d)                               # wrong dtype
    with pytest.raises(ValueError):
        ray_render.get_weights(d.cpu(), d.cpu())                            # host tensors
    with pytest.raises(ValueError):
        ray_render.get_weights(d, dev(8, 4, 1).transpose(0, 1))             # non-contiguous
    with pytest.raises(ValueError):
        ray_render.composite(d, d, d, d, c, dev(4, 8, 6))                   # C % 4 != 0
    with pytest.raises(ValueError):
        ray_render.composite(d, d, d, d, c, dev(4, 8, 2052))                # C above the limit
    with pytest.raises(ValueError):
        ray_render.get_weights(dev(2, 1025, 1), dev(2, 1025, 1))            # S above the ray kernels' limit
    with pytest.raises(ValueError):
        ray_render.FeatureRenderer.forward(dev(2, 257, 4), dev(2, 257, 1))  # S above the feature kernels' limit
    with pytest.raises(ValueError):
        ray_render.composite(d, d, d, dev(4, 7, 1))                         # shapes disagree
    with pytest.raises(ValueError):
        ray_render.get_weights(d, d.clone().requires_grad_(True))           # the bins get no gradient
    with pytest.raises(NotImplementedError):
        ray_render.RGBRenderer()(c, d, ray_indices=torch.zeros(32, dtype=torch.long, device=DEV), num_rays=4)
    with pytest.raises(NotImplementedError):
        ray_render.DepthRenderer("expected")(d, samples, ray_indices=torch.zeros(32, dtype=torch.long, device=DEV), num_rays=4)
    # the C API refuses the same shapes with an error code, before any launch
    import ctypes as C
    nbytes = C.c_int64()
    for n_rays, n_samples, n_channels in ((4, 1025, 0), (4, 257, 4), (4, 8, 6), (4, 8, 2052), (0, 8, 4), (4, 0, 4)):
        desc = _lib.RayDesc(n_rays, n_samples, n_channels, 0, (C.c_float * 3)(0, 0, 0))
        assert _lib.load().pixie_ray_composite_bytes(C.byref(desc), C.byref(nbytes)) != 0, (n_rays, n_samples, n_channels)
    desc = _lib.RayDesc(4, 8, 260, 0, (C.c_float * 3)(0, 0, 0))
    assert _lib.load().pixie_ray_composite_bytes(C.byref(desc), C.byref(nbytes)) == 0 and nbytes.value == 4 * 4 * 2 * 8
