"""torch restatement of one hash-grid MLP with a `dtype` argument, its gradients from autograd: the reference of
tests/test_hashmlp_backward_hip.py.  Written from tests/_field_query_ref.py's formulas (not from the kernels): everything up to the scaled
position q of a level is float32, one rounding per operation; the interpolation weights, gathers, frequency block, layers and
activations run in `dtype`.  float64 is the reference, float32 on the CPU the yardstick whose own distance sets the bar.

    corners(lvls, p32)                 per level: rows (n, 8) int64 and q - floor(q) (n, 3) float32
    params(net, dtype)                 leaf tensors of the net: table, weights, biases
    forward(net, P, p32, extra)        out, the hidden layers' pre-activations and every layer's input
    undecided(net, P, zs, xs)          points with a hidden unit whose float64 pre-activation is within float32's reach of zero
    gradients(net, p32, extra, dY, dtype)   dict(out, table, weights, biases, extra)
    counts(lvls, p32, keep, rows)      contributions per table row from the kept points
    bar(got, ref64, yard32, nets, extra_floor)
"""
import numpy as np
import torch

from tests import _field_query_ref as R

F32 = np.float32


def corners(lvls, p32):
    out = []
    for lv in lvls or []:
        q = R.scaled(p32, lv)
        c0 = np.floor(q)
        w = (q - c0).astype(F32)
        c0 = c0.astype(np.int64)
        rows = np.empty((len(p32), 8), np.int64)
        for corner in range(8):
            o = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
            c = (c0 + o) & 0xFFFFFFFF
            if lv["dense"]:
                idx = (c[:, 0] + c[:, 1] * lv["res"] + c[:, 2] * lv["res"] * lv["res"]) & 0xFFFFFFFF
            else:
                idx = c[:, 0] ^ ((c[:, 1] * R.PRIME_Y) & 0xFFFFFFFF) ^ ((c[:, 2] * R.PRIME_Z) & 0xFFFFFFFF)
            rows[:, corner] = idx % lv["size"] + lv["offset"]
        out.append((rows, w))
    return out


def params(net, dtype, values=None):
    """leaf tensors (requires_grad) of `dtype` on the CPU; `values` (same structure, any tensors / arrays) overrides the net's"""
    src = values or net
    leaf = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).clone().requires_grad_(True)
    biases = src.get("biases") or [None] * len(src["weights"])
    return dict(table=leaf(src.get("table")) if net.get("levels") else None, weights=[leaf(w) for w in src["weights"]], biases=[leaf(b) for b in biases])


def input_row(net, P, p32, extra, dtype):
    parts = []
    for l, (rows, w) in enumerate(corners(net.get("levels"), p32)):
        w = torch.as_tensor(w, dtype=dtype)
        acc = 0
        for corner in range(8):
            wt = torch.ones(len(p32), dtype=dtype)
            for a in range(3):
                wt = wt * (w[:, a] if (corner >> a) & 1 else (1 - w[:, a]))
            acc = acc + wt[:, None] * P["table"][torch.as_tensor(rows[:, corner])]
        parts.append(acc)
    nf = net.get("n_frequencies", 0)
    if nf:
        p = torch.as_tensor(p32, dtype=dtype)
        cols = []
        for j in range(6 * nf):
            dim, octave, phase = j // (2 * nf), (j // 2) % nf, j % 2
            cols.append(torch.sin(float(2 ** octave) * torch.pi * p[:, dim] + phase * (torch.pi / 2)))
        parts.append(torch.stack(cols, dim=1))
    if extra is not None:
        parts.append(extra)
    return torch.cat(parts, dim=1)


def forward(net, P, p32, extra=None, dtype=torch.float64):
    """(out, zs, xs): zs[k] the pre-activation of hidden layer k, xs[i] the input of layer i"""
    x = input_row(net, P, p32, extra, dtype)
    zs, xs = [], []
    last = len(P["weights"]) - 1
    for i, w in enumerate(P["weights"]):
        xs.append(x)
        x = x @ w.T
        if P["biases"][i] is not None:
            x = x + P["biases"][i]
        if i < last:
            zs.append(x)
            x = torch.relu(x)
    act = net.get("act", "none")
    if act == "sigmoid":
        x = 1 / (1 + torch.exp(-x))
    elif act == "exp":
        x = torch.exp(x)
    return x, zs, xs


def undecided(P, zs, xs):
    """(n,) bool from a float64 forward: some hidden unit has |z| < 4 (K + 16) 2^-24 (|W| |x| + |b|), so float32 may decide its ReLU
    the other way"""
    bad = torch.zeros(len(xs[0]), dtype=torch.bool)
    with torch.no_grad():
        for k, z in enumerate(zs):
            w, b = P["weights"][k], P["biases"][k]
            mag = xs[k].abs() @ w.abs().T + (b.abs() if b is not None else 0)
            bad |= (z.abs() < 4 * (w.shape[1] + 16) * 2.0 ** -24 * mag).any(dim=1)
    return bad.numpy()


def gradients(net, p32, extra, dY, dtype, values=None):
    """dY (n, out) numpy, applied as given (zero the undecided rows first).  Returns numpy arrays: out, table, weights, biases, extra."""
    P = params(net, dtype, values)
    e = None if extra is None else torch.as_tensor(extra, dtype=dtype).clone().requires_grad_(True)
    out, _, _ = forward(net, P, p32, e, dtype)
    out.backward(torch.as_tensor(dY, dtype=dtype))
    g = lambda t: None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
    return dict(out=out.detach().numpy(), table=g(P["table"]), weights=[g(w) for w in P["weights"]], biases=[g(b) for b in P["biases"]], extra=g(e))


def counts(lvls, p32, keep, rows):
    m = np.zeros(rows, np.int64)
    for r, _ in corners(lvls, p32):
        m += np.bincount(r[keep].reshape(-1), minlength=rows)
    return m


def floor_of(ref64, nets):
    k = sum(sum(R.fan_ins(n)) for n in nets) + 16
    return k * 2.0 ** -24 * max(1.0, float(np.max(np.abs(ref64), initial=0.0)))


def bar(ref64, yard32, nets, extra_floor=0.0):
    """per-element bound on |got - ref64|: 3 x max |yardstick32 - ref64| + (sum of fan-ins + 16) 2^-24 max(1, max |ref64|), plus
    `extra_floor` (scalar or array: the table gradient's m_r 2^-s)"""
    return 3.0 * float(np.max(np.abs(yard32.astype(np.float64) - ref64), initial=0.0)) + floor_of(ref64, nets) + extra_floor
