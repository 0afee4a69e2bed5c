"""torch restatement of the proposal density field (pixie_amd.density_field, csrc/density_field.hip) with a `dtype` argument, written
from the reference module's lines (nerfstudio fields/density_fields.py:94-117) over the helpers the 64-wide tests already use:

    front end   _field_query_ref.world_to_unit (float32, one rounding per operation), positions * selector
    network     _hashmlp_grad_ref.forward / undecided / bar, which do not care about the width
    on top      density = average_init_density * trunc_exp(h) * selector in `dtype`; trunc_exp's backward is g exp(clamp(h, -15, 15))

float64 is the reference, float32 on the CPU the yardstick whose own distance sets the bar.

    random_net(rng, convention, ...)        a 16-wide net with _field_query_ref.random_net's initialisation
    undecided(net, x32, front)              ReLU kinks, from the float64 forward alone
    evaluate(net, x32, dD, dtype, front)    dict(h, density, table, weights, biases, p, selector)
"""
import math

import numpy as np
import torch

from tests import _field_query_ref as R
from tests import _hashmlp_grad_ref as G

F32 = np.float32
WIDTH = 16


def random_net(rng, convention, num_levels, base_res, max_res, log2_T, F=2, n_hidden=1, bias=True):
    lvls, rows = R.levels(convention, num_levels, base_res, max_res, log2_T)
    dims = [num_levels * F] + [WIDTH] * n_hidden + [1]
    weights = [(rng.standard_normal((dims[i + 1], dims[i])) * math.sqrt(2.0 / dims[i])).astype(F32) for i in range(len(dims) - 1)]
    biases = [(0.3 * rng.standard_normal(dims[i + 1])).astype(F32) for i in range(len(dims) - 1)] if bias else None
    table = rng.uniform(-1, 1, (rows, F)).astype(F32)
    return dict(levels=lvls, table=table, weights=weights, biases=biases, n_frequencies=0, n_extra=0, act="none", rows=rows, F=F,
                convention=convention, config=dict(num_levels=num_levels, base_res=base_res, max_res=max_res, log2_hashmap_size=log2_T,
                                                   features_per_level=F, num_layers=n_hidden + 1, use_linear=n_hidden == 0))


class TruncExp(torch.autograd.Function):
    """field_components/activations.py:28-41"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, min=-15, max=15))


def front_end(x32, front):
    """front: dict(contraction, aabb=None, world_to_nerf=None).  Returns (masked unit positions float32, selector bool)."""
    A = front.get("world_to_nerf")
    A = np.eye(4, dtype=F32)[:3] if A is None else np.asarray(A, F32)[:3]
    with np.errstate(invalid="ignore"):
        p, sel = R.world_to_unit(np.asarray(x32, F32), A, front.get("contraction", True), front.get("aabb"))
    masked = np.where(sel[:, None], p, F32(0)).astype(F32)      # NaN * 0 would be NaN: the device gives such a point p = 0
    return masked, sel


def undecided(net, x32, front):
    masked, sel = front_end(x32, front)
    P = G.params(net, torch.float64)
    with torch.no_grad():
        _, zs, xs = G.forward(net, P, masked, None, torch.float64)
    if not zs:
        return np.zeros(len(masked), bool)
    return G.undecided(P, zs, xs) & sel


def evaluate(net, x32, dD, dtype, front, average_init_density=1.0, values=None):
    """dD (n,) = dL/d density, applied as given.  numpy arrays: h (n,), density (n,), table, weights, biases gradients."""
    masked, sel = front_end(x32, front)
    P = G.params(net, dtype, values)
    h, _, _ = G.forward(net, P, masked, None, dtype)
    h = h[:, 0]
    density = average_init_density * TruncExp.apply(h) * torch.as_tensor(sel, dtype=dtype)
    density.backward(torch.as_tensor(dD, dtype=dtype))
    g = lambda t: None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
    return dict(h=h.detach().numpy(), density=density.detach().numpy(), table=g(P["table"]), weights=[g(w) for w in P["weights"]],
                biases=[g(b) for b in P["biases"]], p=masked, selector=sel)
