"""Torch restatement of what gaussian-splatting/train.py does with the gradients of an iteration, for any dtype on the CPU:

    stats_ref()                 train.py:114-116 (max_radii2D, add_densification_stats)
    densify_ref()               scene/gaussian_model.py:densify_and_prune (:393-405) with the split's normal draw z as an input
    replace_tensor_to_optimizer / prune_optimizer / cat_tensors_to_optimizer
                                the reference's optimiser surgery (gaussian_model.py:262-331) on a bare optimiser
    make_case() / CASES         the populations of tests/golden/gs_densify.npz and of the synthetic GPU cases
    margins()                   how far every decision of a case lies from its threshold, relative

densify_ref follows the reference pass by pass (clone, split, prune of the split parents, final prune) on index arrays, so its row
order is the reference's by construction; tests/test_gs_optim_ref.py pins it to the golden the reference itself wrote.
"""
import numpy as np
import torch
from torch import nn

FIELDS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
EXTENT = 5.0
PERCENT_DENSE = 0.01
MAX_GRAD = 0.0002
MIN_OPACITY = 0.005
MAX_SCREEN_SIZE = 20

# name -> (n, sh_degree, max_screen_size, population)
GOLDEN_CASES = {"mixed": (96, 3, MAX_SCREEN_SIZE, "mixed"), "nothing_selected": (40, 3, MAX_SCREEN_SIZE, "quiet"),
                "no_screen_size": (64, 3, None, "mixed"), "degree0": (50, 0, MAX_SCREEN_SIZE, "mixed")}
SYNTHETIC_CASES = {"n1": (1, 3, MAX_SCREEN_SIZE, "split_only"), "n63": (63, 3, MAX_SCREEN_SIZE, "mixed"),
                   "n257": (257, 3, MAX_SCREEN_SIZE, "mixed"), "n4099": (4099, 3, MAX_SCREEN_SIZE, "mixed"),
                   "all_pruned": (70, 3, MAX_SCREEN_SIZE, "faint"), "nothing_cloned": (130, 3, MAX_SCREEN_SIZE, "no_clone"),
                   "nothing_split": (130, 0, None, "no_split")}
CASES = {**GOLDEN_CASES, **SYNTHETIC_CASES}


def make_case(name):
    """float32 numpy state of one case: the six parameters, their moments (zero here: the golden generator replaces parameters
    and moments by what one optimizer.step() of the reference leaves), the statistics and z for the largest possible split."""
    n, degree, mss, pop = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + n)
    dense_thr, world_thr = PERCENT_DENSE * EXTENT, 0.1 * EXTENT
    k = (degree + 1) ** 2

    # gradient class: 0 quiet (g well below max_grad), 1 loud, 2 denom == 0 and accum == 0 (NaN -> 0), 3 denom == 0 and accum > 0 (inf)
    # size class: 0 small (clone range), 1 middle (split, children stay), 2 large (split, children stay, parent over the world
    #             threshold), 3 huge (children over the world threshold too)
    # opacity class: 0 faint (pruned), 1 solid
    if pop == "mixed":
        grad_cls = rng.choice([0, 1, 2, 3], size=n, p=[0.4, 0.45, 0.1, 0.05])
        size_cls = rng.choice([0, 1, 2, 3], size=n, p=[0.4, 0.3, 0.15, 0.15])
        op_cls = rng.choice([0, 1], size=n, p=[0.25, 0.75])
        if n >= 40:         # every kind the issue names is present, whatever the draw
            forced = [(1, 0, 1), (1, 1, 1), (0, 0, 0), (0, 2, 1), (0, 0, 1), (2, 1, 1), (1, 0, 0), (1, 3, 1), (1, 2, 1), (3, 1, 1), (1, 1, 0)]
            for j, (g, s, o) in enumerate(forced):
                grad_cls[3 * j + 1], size_cls[3 * j + 1], op_cls[3 * j + 1] = g, s, o
    elif pop == "quiet":
        grad_cls = rng.choice([0, 2], size=n)
        size_cls = rng.choice([0, 1], size=n)
        op_cls = rng.choice([0, 1], size=n, p=[0.2, 0.8])
    elif pop == "split_only":
        grad_cls, size_cls, op_cls = np.full(n, 1), np.full(n, 1), np.full(n, 1)
    elif pop == "faint":
        grad_cls = rng.choice([0, 1], size=n)
        size_cls = rng.choice([0, 1, 2], size=n)
        op_cls = np.zeros(n, dtype=np.int64)
    elif pop == "no_clone":
        grad_cls = rng.choice([0, 1], size=n)
        size_cls = np.where(grad_cls == 1, rng.choice([1, 2, 3], size=n), rng.choice([0, 1, 2, 3], size=n))
        op_cls = rng.choice([0, 1], size=n, p=[0.25, 0.75])
    elif pop == "no_split":
        grad_cls = rng.choice([0, 1, 2], size=n)
        size_cls = np.where(grad_cls == 1, 0, rng.choice([0, 1, 2], size=n))
        op_cls = rng.choice([0, 1], size=n, p=[0.25, 0.75])
    else:
        raise KeyError(pop)

    g = np.where(grad_cls == 1, MAX_GRAD * rng.uniform(1.5, 4.0, n), MAX_GRAD * rng.uniform(0.1, 0.8, n))
    den = rng.integers(1, 6, n).astype(np.float64)
    acc = g * den
    den[grad_cls >= 2] = 0.0
    acc[grad_cls == 2] = 0.0
    smax = np.select([size_cls == 0, size_cls == 1, size_cls == 2], [dense_thr * rng.uniform(0.3, 0.8, n), rng.uniform(2 * dense_thr, 0.6 * world_thr, n),
                                                                     world_thr * rng.uniform(1.2, 1.4, n)], world_thr * rng.uniform(2.0, 3.0, n))
    scale = smax[:, None] * rng.uniform(0.2, 0.9, (n, 3))
    scale[np.arange(n), rng.integers(0, 3, n)] = smax
    prob = np.where(op_cls == 0, rng.uniform(0.001, 0.003, n), rng.uniform(0.02, 0.99, n))
    out = {
        "xyz": rng.normal(0, 2, (n, 3)), "f_dc": rng.normal(0, 1, (n, 1, 3)), "f_rest": rng.normal(0, 0.2, (n, k - 1, 3)),
        "opacity": np.log(prob / (1 - prob))[:, None], "scaling": np.log(scale), "rotation": rng.normal(0, 1, (n, 4)),
        "xyz_gradient_accum": acc[:, None], "denom": den[:, None], "max_radii2D": rng.choice([0.0, 3.0, 17.0, 45.0, 80.0], n),
        "z": rng.normal(0, 1, (2 * n, 3)),
    }
    out = {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}
    for f in FIELDS:
        out["exp_avg." + f] = np.zeros_like(out[f])
        out["exp_avg_sq." + f] = np.zeros_like(out[f])
    return out


def margins(state, max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=EXTENT, percent_dense=PERCENT_DENSE):
    """The smallest relative distance |q / threshold - 1| over the rows, at float64, of: g against max_grad, max(exp(scaling))
    against percent_dense * extent and against 0.1 * extent (the split children's too), sigmoid(opacity) against min_opacity."""
    t = {k: torch.as_tensor(np.asarray(v)).double() for k, v in state.items() if k in ("xyz_gradient_accum", "denom", "scaling", "opacity")}
    g = (t["xyz_gradient_accum"] / t["denom"]).squeeze(-1)
    g[g.isnan()] = 0.0
    smax = t["scaling"].exp().max(dim=1).values
    prob = torch.sigmoid(t["opacity"]).squeeze(-1)
    rel = lambda q, thr: float(((q / thr) - 1).abs().min()) if q.numel() else float("inf")
    return {"grad": rel(g, max_grad), "dense": rel(smax, percent_dense * extent), "world": rel(smax, 0.1 * extent),
            "world_children": rel(smax / 1.6, 0.1 * extent), "opacity": rel(prob, min_opacity)}


def build_rotation(r):
    """rotation matrices (n, 3, 3) of the normalised quaternions (w, x, y, z), the convention of utils/general_utils.py"""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q.unbind(dim=1)
    rows = [torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], dim=1),
            torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], dim=1),
            torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1)]
    return torch.stack(rows, dim=1)


def stats_ref(xyz_gradient_accum, denom, max_radii2D, viewspace_grad, radii):
    """train.py:114-116; returns the three new arrays"""
    vis = radii > 0
    max_radii2D = max_radii2D.clone()
    accum, denom = xyz_gradient_accum.clone(), denom.clone()
    max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis].to(max_radii2D.dtype))
    accum[vis] += torch.norm(viewspace_grad[vis, :2], dim=-1, keepdim=True)
    denom[vis] += 1
    return accum, denom, max_radii2D


def densify_ref(state, max_grad, min_opacity, extent, percent_dense, max_screen_size, z, dtype=torch.float32):
    """`state`: the arrays of make_case() (numpy or torch).  Returns a dict: the six parameters, "exp_avg.<f>", "exp_avg_sq.<f>",
    the three zeroed statistics, "source_index" (int64), "counts" (kept, clones kept, children kept, pruned) and "n_split"."""
    t = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items() if k != "z"}
    z = torch.as_tensor(np.asarray(z)).to(dtype)
    n = t["xyz"].shape[0]
    grads = t["xyz_gradient_accum"] / t["denom"]
    grads[grads.isnan()] = 0.0
    get_scaling = torch.exp(t["scaling"])
    smax = get_scaling.max(dim=1).values

    # densify_and_clone
    clone_mask = (torch.norm(grads, dim=-1) >= max_grad) & (smax <= percent_dense * extent)
    clone_src = torch.nonzero(clone_mask).squeeze(-1)
    # densify_and_split: the padded gradient is zero for the clones, so only originals are selected
    split_mask = (grads.squeeze(-1) >= max_grad) & (smax > percent_dense * extent)
    split_src = torch.nonzero(split_mask).squeeze(-1)
    n_split = int(split_src.numel())
    if z.shape[0] != 2 * n_split:
        raise ValueError(f"z must be (2 * {n_split}, 3), got {tuple(z.shape)}")
    stds = get_scaling[split_src].repeat(2, 1)
    samples = torch.zeros_like(stds) + stds * z
    rots = build_rotation(t["rotation"][split_src]).repeat(2, 1, 1)
    child_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][split_src].repeat(2, 1)
    child_scaling = torch.log(get_scaling[split_src].repeat(2, 1) / (0.8 * 2))

    keep_orig = torch.nonzero(~split_mask).squeeze(-1)
    source = torch.cat([keep_orig, clone_src, split_src, split_src])
    n_a, n_b = keep_orig.numel(), clone_src.numel()
    new = {f: t[f][source].clone() for f in FIELDS}
    new["xyz"][n_a + n_b:] = child_xyz
    new["scaling"][n_a + n_b:] = child_scaling
    fresh = torch.ones(source.numel(), dtype=torch.bool)
    fresh[:n_a] = False
    for f in FIELDS:
        for mom in ("exp_avg.", "exp_avg_sq."):
            m = t[mom + f][source].clone()
            m[fresh] = 0
            new[mom + f] = m

    # final prune; max_radii2D is all zero here (densification_postfix), so `max_radii2D > max_screen_size` never fires
    prune = (torch.sigmoid(new["opacity"]) < min_opacity).squeeze(-1)
    if max_screen_size:
        prune = prune | (torch.zeros(source.numel(), dtype=dtype) > max_screen_size) | (torch.exp(new["scaling"]).max(dim=1).values > 0.1 * extent)
    keep = ~prune
    out = {k: v[keep] for k, v in new.items()}
    m_rows = int(keep.sum())
    out["source_index"] = source[keep]
    seg = torch.zeros(source.numel(), dtype=torch.int64)
    seg[n_a:n_a + n_b] = 1
    seg[n_a + n_b:] = 2
    kept_seg = seg[keep]
    out["counts"] = (int((kept_seg == 0).sum()), int((kept_seg == 1).sum()), int((kept_seg == 2).sum()), int(prune.sum()))
    out["n_split"] = n_split
    out["xyz_gradient_accum"] = torch.zeros((m_rows, 1), dtype=dtype)
    out["denom"] = torch.zeros((m_rows, 1), dtype=dtype)
    out["max_radii2D"] = torch.zeros((m_rows,), dtype=dtype)
    return out


def split_count(state, max_grad=MAX_GRAD, extent=EXTENT, percent_dense=PERCENT_DENSE):
    g = torch.as_tensor(state["xyz_gradient_accum"]).double() / torch.as_tensor(state["denom"]).double()
    g[g.isnan()] = 0.0
    smax = torch.as_tensor(state["scaling"]).double().exp().max(dim=1).values
    return int(((g.squeeze(-1) >= max_grad) & (smax > percent_dense * extent)).sum())


# ---- the reference's optimiser surgery (gaussian_model.py:262-331), on a bare optimiser whose groups carry "name" ----
# What the three reference methods have in common, and what an optimiser must allow: the state of a group's only parameter is
# looked up with optimizer.state.get(), its dict is mutated in place ("exp_avg", "exp_avg_sq" replaced, "step" untouched), removed
# from optimizer.state under the old parameter and stored under a new nn.Parameter, which also replaces group["params"][0].
def _rekey(optimizer, group, value, moments):
    old = group["params"][0]
    state = optimizer.state.get(old, None)
    param = nn.Parameter(value.requires_grad_(True))
    if state is not None:
        state["exp_avg"], state["exp_avg_sq"] = moments(state)
        del optimizer.state[old]
        optimizer.state[param] = state
    group["params"][0] = param
    return param


def replace_tensor_to_optimizer(optimizer, tensor, name):
    """one group's tensor replaced, its moments zeroed (the reference requires the state to exist)"""
    out = {}
    for group in optimizer.param_groups:
        if group["name"] == name:
            assert optimizer.state.get(group["params"][0], None) is not None
            out[name] = _rekey(optimizer, group, tensor, lambda st: (torch.zeros_like(tensor), torch.zeros_like(tensor)))
    return out


def prune_optimizer(optimizer, mask):
    """every group's tensor and moments filtered by a row mask"""
    return {group["name"]: _rekey(optimizer, group, group["params"][0][mask], lambda st: (st["exp_avg"][mask], st["exp_avg_sq"][mask]))
            for group in optimizer.param_groups}


def cat_tensors_to_optimizer(optimizer, tensors_dict):
    """every group's tensor extended by rows, its moments by zeros"""
    out = {}
    for group in optimizer.param_groups:
        assert len(group["params"]) == 1
        ext = tensors_dict[group["name"]]
        grow = lambda st, ext=ext: (torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0), torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0))
        out[group["name"]] = _rekey(optimizer, group, torch.cat((group["params"][0], ext), dim=0), grow)
    return out
