"""GPU checks of the differentiable hash-grid MLP (pixie_amd.field_training, pixie_amd/csrc/field_query_backward.hip) against the
float64 torch restatement of tests/_hashmlp_grad_ref.py, whose gradients come from autograd.

Bar, for every gradient array: max |got - ref64| <= 3 x max |yardstick32 - ref64| + floor, the yardstick being the same restatement in
float32 on the CPU and the floor (sum of fan-ins + 16) 2^-24 max(1, max |ref64|) (_field_query_ref.bar's form).  The table gradient
alone gets m_r 2^-s more per row: m_r contributions (counted by the restatement) of at most 2^(-s-1) quantisation error each, s read
back from the scratch header.

ReLU kinks.  A hidden unit whose float64 pre-activation has |z| < 4 (K + 16) 2^-24 (|W| |x| + |b|) may fire differently in float32.
Points with such a unit get their dY row zeroed on both sides, so they contribute to no gradient whatever the kernel decided; at most
5 % of a case's points may be zeroed, asserted from the reference alone.

The measured ratios are appended to the file named by PIXIE_HASHMLP_PARITY_OUT when it is set (profiles/hashmlp_grad_parity.txt is
such a run's output).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _field_query_ref as R
from tests import _hashmlp_grad_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 200
OUT = 80                     # ragged against the 64-column chunk of the output layer

# name -> (convention, log2_T, F, n_frequencies, n_extra, n_hidden, out_dim, bias, activation, n_levels, base_res, max_res)
NETS = {
    "tcnn_F2": ("tcnn", 8, 2, 0, 0, 2, OUT, True, "none", 4, 4, 32),
    "tcnn_F4": ("tcnn", 8, 4, 0, 0, 2, OUT, True, "none", 4, 4, 32),
    "tcnn_F8": ("tcnn", 8, 8, 0, 0, 2, OUT, True, "none", 4, 4, 32),
    "ns_F2": ("nerfstudio", 8, 2, 0, 0, 2, OUT, True, "none", 4, 4, 32),
    "ns_F4": ("nerfstudio", 8, 4, 0, 0, 2, OUT, True, "none", 4, 4, 32),
    "ns_F8": ("nerfstudio", 8, 8, 0, 0, 2, OUT, True, "none", 4, 4, 32),
    "tcnn_F2_h1": ("tcnn", 8, 2, 0, 0, 1, OUT, True, "none", 4, 4, 32),
    "tcnn_F2_h4": ("tcnn", 8, 2, 0, 0, 4, OUT, True, "none", 4, 4, 32),
    "ns_F4_h2_nobias": ("nerfstudio", 8, 4, 0, 0, 2, OUT, False, "none", 4, 4, 32),
    "tcnn_F8_freq6": ("tcnn", 8, 8, 6, 0, 2, OUT, True, "none", 4, 4, 32),               # 68 columns: two chunks of dX, one of them mixed
    "tcnn_F2_extra15": ("tcnn", 8, 2, 0, 15, 2, OUT, True, "none", 4, 4, 32),            # extra requires grad
    "color_head_sigmoid": (None, 0, 0, 0, 15, 2, 3, True, "sigmoid", 0, 0, 0),           # no grid
    "tcnn_F2_exp": ("tcnn", 8, 2, 0, 0, 1, 16, True, "exp", 4, 4, 32),
    "tcnn_F2_out1": ("tcnn", 8, 2, 0, 0, 1, 1, True, "none", 4, 4, 32),
    "feature_net_out768": ("tcnn", 10, 8, 6, 0, 2, 768, False, "none", 12, 16, 128),     # the reference feature net's 132 columns
    "tcnn_T4_collisions": ("tcnn", 4, 2, 0, 0, 1, 16, True, "none", 4, 4, 32),           # 16-row levels: every row hit from every level
    "ns_T4_collisions": ("nerfstudio", 4, 4, 0, 0, 1, 16, True, "none", 4, 4, 32),
}
_cases = {}


def note(line):
    print(line)
    path = os.environ.get("PIXIE_HASHMLP_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def make_net(name):
    conv, T, F, nf, ne, nh, out, bias, act, L, lo, hi = NETS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    lv, rows = R.levels(conv, L, lo, hi, T) if conv else (None, 0)
    return R.random_net(rng, lv, rows, F, nf, ne, nh, out, bias, act), rows, rng


def prepare(net, rows, p, extra, dY):
    """zeroes the undecided points' dY rows; returns (dY, keep, ref64, yard32, m_r): computed from the restatement alone"""
    P = G.params(net, torch.float64)
    with torch.no_grad():
        _, zs, xs = G.forward(net, P, p, None if extra is None else torch.as_tensor(extra, dtype=torch.float64))
    bad = G.undecided(P, zs, xs)
    assert bad.mean() <= 0.05, f"{bad.mean():.3f} of the points sit on a ReLU kink"
    dY = dY.copy()
    dY[bad] = 0
    ref = G.gradients(net, p, extra, dY, torch.float64)
    yard = G.gradients(net, p, extra, dY, torch.float32)
    m_r = G.counts(net["levels"], p, ~bad, rows) if net["levels"] else None
    return dY, ~bad, ref, yard, m_r


def case(name, n=N):
    if (name, n) not in _cases:
        net, rows, rng = make_net(name)
        p = rng.random((n, 3)).astype(np.float32)
        p[:min(n, 4)] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0.25, 0.75, 0.5]][:min(n, 4)]      # cell boundaries: zero-weight corners
        extra = rng.standard_normal((n, net["n_extra"])).astype(np.float32) if net["n_extra"] else None
        dY = rng.standard_normal((n, np.shape(net["weights"][-1])[0])).astype(np.float32)
        _cases[(name, n)] = (net, rows, p, extra) + prepare(net, rows, p, extra, dY)
    return _cases[(name, n)]


def device_module(net):
    from pixie_amd import field_query as FQ, field_training as FT
    lv = None
    if net["levels"]:
        lv = np.array([tuple(l[k] for k in FQ.LEVEL_DTYPE.names) for l in net["levels"]], FQ.LEVEL_DTYPE)
    return FT.TrainableHashMLP(lv, net["table"], net["weights"], net["biases"], net["n_frequencies"], net["n_extra"], net["act"], device=DEV)


def last_shift():
    from pixie_amd import field_training as FT
    head = FT._HashMlpFunction.last_header.cpu().numpy().view(np.int32)
    return int(head[1]), int(head[2])


def module_gradients(net, p, extra, dY, module=None):
    m = module or device_module(net)
    m.zero_grad(set_to_none=True)
    pos = torch.from_numpy(p).to(DEV) if (net["levels"] or net["n_frequencies"]) else None
    e = None if extra is None else torch.from_numpy(extra).to(DEV).requires_grad_(True)
    out = m(pos, e)
    out.backward(torch.from_numpy(dY).to(DEV))
    s, state = last_shift() if net["levels"] else (0, 1)
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return dict(out=host(out), table=host(m.table.grad) if m.table is not None else None, weights=[host(w.grad) for w in m.weights],
                biases=[host(b.grad) if b is not None else None for b in m.bias_list()], extra=host(e.grad) if e is not None else None,
                s=s, state=state, module=m, pos=pos)


def arrays(g):
    yield "d_table", g["table"]
    for i, w in enumerate(g["weights"]):
        yield f"d_weight[{i}]", w
    for i, b in enumerate(g["biases"]):
        yield f"d_bias[{i}]", b
    yield "d_extra", g["extra"]


def within(got, ref, yard, net, m_r, what, only=None):
    for (name, a), (_, r), (_, y) in zip(arrays(got), arrays(ref), arrays(yard)):
        if r is None or (only and not name.startswith(only)):
            assert r is not None or a is None, name
            continue
        assert a is not None and a.shape == r.shape and np.all(np.isfinite(a)), f"{what} {name}"
        extra = m_r[:, None] * 2.0 ** -got["s"] if name == "d_table" else 0.0
        err = np.abs(a.astype(np.float64) - r)
        limit = G.bar(r, y, [net], extra)
        yd = float(np.abs(y.astype(np.float64) - r).max())
        note(f"{what} {name}: max|got - f64| {err.max():.3e}, float32 CPU {yd:.3e} (ratio {err.max() / yd if yd else float('inf'):.2f}), "
             f"bar {float(np.min(limit)):.3e}" + (f", s {got['s']}" if name == "d_table" else ""))
        assert np.all(err <= limit), f"{what} {name}"


# ---- 1. gradients against float64 ------------------------------------------------------------------------------------------------
N_COLLIDE = 600             # uniform points into 16-row levels: some 300 contributions per row


@pytest.mark.parametrize("name", list(NETS))
def test_gradients_against_float64(name):
    net, rows, p, extra, dY, keep, ref, yard, m_r = case(name, N_COLLIDE if "collisions" in name else N)
    if "collisions" in name:
        assert m_r.min() >= 100 and rows <= 64, (name, m_r.min(), rows)
    got = module_gradients(net, p, extra, dY)
    plain = got["module"].to_hashmlp()(got["pos"], None if extra is None else torch.from_numpy(extra).to(DEV))
    assert np.array_equal(got["out"].view(np.uint32), plain.cpu().numpy().view(np.uint32)), "the training forward carries HashMLP.__call__'s bits"
    if net["levels"]:
        assert got["state"] == 0
    within(got, ref, yard, net, m_r, name)


# ---- 2. tile edges, through the C boundary ----------------------------------------------------------------------------------------
CANARY = 64


def guarded(shape, fill=float("nan")):
    """a float32 device tensor of `shape` inside a buffer whose tail holds a canary"""
    count = int(np.prod(shape))
    buf = torch.full((count + CANARY,), fill, dtype=torch.float32, device=DEV)
    buf[count:] = 12345.0
    return buf, buf[:count].view(*shape)


def intact(buf):
    return bool((buf[-CANARY:] == 12345.0).all())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges_with_canaries(n):
    from pixie_amd import _lib, field_training as FT
    name = "tcnn_F2_extra15"
    net, rows, p, extra, dY, keep, ref, yard, m_r = case(name, n)
    h = device_module(net).to_hashmlp()
    desc = h.desc()
    saved_bytes, scratch_bytes = FT.train_bytes(desc, n)
    assert saved_bytes == 4 * n * (h.in_dim + 64 * h.n_hidden)
    pos, ext, dy = (torch.from_numpy(a).to(DEV) for a in (p, extra, dY))
    out_buf, out = guarded((n, h.out_dim))
    saved_buf, saved = guarded((saved_bytes // 4,))
    lib, stream = _lib.load(), _lib.current_stream_ptr()
    _lib.check(lib.pixie_hashmlp_forward_saved(C.byref(desc), pos.data_ptr(), ext.data_ptr(), n, out.data_ptr(), saved.data_ptr(), stream), "forward_saved")
    assert torch.equal(out, h(pos, ext)) and bool(torch.isfinite(saved).all()) and intact(out_buf) and intact(saved_buf)
    g = _lib.HashMlpGrads()
    bufs = {"table": guarded(tuple(h.table.shape)), "extra": guarded((n, h.n_extra))}
    g.d_table, g.d_extra = bufs["table"][1].data_ptr(), bufs["extra"][1].data_ptr()
    for i, (w, b) in enumerate(zip(h.weights, h.biases)):
        bufs[f"w{i}"], bufs[f"b{i}"] = guarded(tuple(w.shape)), guarded(tuple(b.shape))
        g.d_weight[i], g.d_bias[i] = bufs[f"w{i}"][1].data_ptr(), bufs[f"b{i}"][1].data_ptr()
    scratch = torch.zeros(scratch_bytes + 256 + 4 * CANARY, dtype=torch.uint8, device=DEV)
    at = (-scratch.data_ptr()) % 256
    scratch[at + scratch_bytes:] = 77
    _lib.check(lib.pixie_hashmlp_backward(C.byref(desc), pos.data_ptr(), ext.data_ptr(), n, out.data_ptr(), saved.data_ptr(), dy.data_ptr(), C.byref(g),
                                          scratch.data_ptr() + at, stream), "backward")
    torch.cuda.synchronize()
    assert all(intact(b) for b, _ in bufs.values()) and bool((scratch[at + scratch_bytes:] == 77).all()), "a write past a buffer's end"
    head = scratch[at:at + 12].cpu().numpy().view(np.int32)
    host = lambda k: bufs[k][1].cpu().numpy()
    got = dict(table=host("table"), weights=[host(f"w{i}") for i in range(len(h.weights))], biases=[host(f"b{i}") for i in range(len(h.weights))],
               extra=host("extra"), s=int(head[1]))
    within(got, ref, yard, net, m_r, f"{name} n={n}")


# ---- 3. collisions -----------------------------------------------------------------------------------------------------------------
def test_thousand_copies_of_one_point():
    name, copies = "tcnn_F2", 1000
    net, rows, rng = make_net(name)
    p1 = np.array([[0.3371, 0.7213, 0.5532]], np.float32)
    dY1 = rng.standard_normal((1, OUT)).astype(np.float32)
    dY1, keep, one, _, _ = prepare(net, rows, p1, None, dY1)
    assert keep.all(), "the point sits on a ReLU kink: pick another"
    p, dY = np.repeat(p1, copies, axis=0), np.repeat(dY1, copies, axis=0)
    yard = G.gradients(net, p, None, dY, torch.float32)
    m_r = G.counts(net["levels"], p, np.ones(copies, bool), rows)
    got = module_gradients(net, p, None, dY)
    ref = dict(one, table=copies * one["table"], weights=[copies * w for w in one["weights"]], biases=[copies * b for b in one["biases"]])
    assert (m_r > 0).sum() <= 8 * 4 and m_r.max() >= copies
    within(got, ref, yard, net, m_r, "1000 copies", only="d_table")
    assert np.all(got["table"][m_r == 0] == 0)
    perm = rng.permutation(copies)
    again = module_gradients(net, p[perm], None, dY[perm])
    assert np.array_equal(got["table"].view(np.uint32), again["table"].view(np.uint32))


# (the 16-row levels of NETS["*_T4_collisions"] run through test_gradients_against_float64 with N_COLLIDE points)


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tcnn_F8_freq6", "tcnn_F2_extra15", "ns_T4_collisions"])
def test_runs_and_permutations(name):
    net, rows, p, extra, dY, keep, ref, yard, m_r = case(name, N_COLLIDE if "collisions" in name else N)
    a = module_gradients(net, p, extra, dY)
    b = module_gradients(net, p, extra, dY)
    for (what, x), (_, y) in zip(arrays(a), arrays(b)):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"two runs differ in {what}"
    perm = np.random.default_rng(5).permutation(len(p))
    c = module_gradients(net, p[perm], None if extra is None else extra[perm], dY[perm])
    assert np.array_equal(a["table"].view(np.uint32), c["table"].view(np.uint32)), "the table gradient depends on the order of the points"
    if extra is not None:
        assert np.array_equal(a["extra"][perm].view(np.uint32), c["extra"].view(np.uint32)), "a point's d_extra depends on its tile mates"
        c["extra"] = c["extra"][np.argsort(perm)]
    within(c, ref, yard, net, m_r, f"{name} permuted")


# ---- 5. exponent edges ------------------------------------------------------------------------------------------------------------
def test_exponent_edges():
    name = "tcnn_F2_extra15"
    net, rows, p, extra, dY, keep, ref, yard, m_r = case(name)
    zero = module_gradients(net, p, extra, np.zeros_like(dY))
    assert zero["state"] == 1
    for what, a in arrays(zero):
        assert a is not None and not a.any(), f"dY = 0 leaves {what} non-zero"
    base = module_gradients(net, p, extra, dY)
    for power in (-100, 100):
        scaled = module_gradients(net, p, extra, np.ldexp(dY, power).astype(np.float32))
        assert scaled["state"] == 0 and scaled["s"] == base["s"] - power
        want = np.ldexp(base["table"], power).astype(np.float32)
        assert np.all(np.isfinite(want)) and np.all((want != 0) == (base["table"] != 0)), "the scaled gradient must not leave float32's range"
        assert np.array_equal(scaled["table"].view(np.uint32), want.view(np.uint32)), f"2^{power}"
    bad = dY.copy()
    bad[int(np.flatnonzero(keep)[3]), 7] = np.inf
    inf = module_gradients(net, p, extra, bad)               # the call itself succeeded: module_gradients checks the return code
    assert inf["state"] == 2 and np.isnan(inf["table"]).all(), "one Inf in dY: the whole table gradient is NaN"


# ---- 6. chain: density net -> geometry columns -> colour head ------------------------------------------------------------------------
def test_chain_density_to_color():
    rng = np.random.default_rng(77)
    lv, rows = R.levels("tcnn", 4, 4, 32, 8)
    dnet = R.random_net(rng, lv, rows, 2, n_hidden=1, out_dim=16)
    cnet = R.random_net(rng, n_extra=15, n_hidden=2, out_dim=3, act="sigmoid")
    p = rng.random((N, 3)).astype(np.float32)
    r = rng.standard_normal((N, 3)).astype(np.float32)

    def restated(dtype, r_rows, find_kinks=False):
        Pd, Pc = G.params(dnet, dtype), G.params(cnet, dtype)
        h, zd, xd = G.forward(dnet, Pd, p, None, dtype)
        rgb, zc, xc = G.forward(cnet, Pc, p, h[:, 1:], dtype)
        if find_kinks:
            return G.undecided(Pd, zd, xd) | G.undecided(Pc, zc, xc)
        (rgb * torch.as_tensor(r_rows, dtype=dtype)).sum().backward()
        g = lambda t: None if t is None else t.grad.numpy()
        return dict(table=g(Pd["table"]), weights=[g(w) for w in Pd["weights"]], biases=[g(b) for b in Pd["biases"]], extra=None)

    bad = restated(torch.float64, r, True)
    assert bad.mean() <= 0.05
    r[bad] = 0
    ref, yard = restated(torch.float64, r), restated(torch.float32, r)
    dm, cm = device_module(dnet), device_module(cnet)
    h = dm(torch.from_numpy(p).to(DEV))
    rgb = cm(None, h[:, 1:])
    (rgb * torch.from_numpy(r).to(DEV)).sum().backward()
    # the density net's backward ran last: its header is the one in reach
    s, state = last_shift()
    host = lambda t: t.grad.cpu().numpy()
    got = dict(table=host(dm.table), weights=[host(w) for w in dm.weights], biases=[host(b) for b in dm.bias_list()], extra=None, s=s)
    assert state == 0
    within(got, ref, yard, dnet, G.counts(lv, p, ~bad, rows), "chain (density net)")
    # the bar's fan-ins are the density net's alone: the colour head's roundings reach it through d_extra, which the yardstick carries


# ---- 7. it trains -----------------------------------------------------------------------------------------------------------------
def test_it_trains():
    rng = np.random.default_rng(11)
    lv, rows = R.levels("tcnn", 2, 8, 16, 12)
    net = R.random_net(rng, lv, rows, 2, n_hidden=1, out_dim=3)
    net["table"] = (net["table"] * 0.1).astype(np.float32)
    p = rng.random((4096, 3)).astype(np.float32)
    x, y, z = (p[:, a].astype(np.float64) for a in range(3))
    target = np.stack([np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y), z * z, x * y + 0.5 * np.sin(3 * z)], axis=1).astype(np.float32)
    steps = 150

    P = G.params(net, torch.float32)
    leaves = [P["table"]] + P["weights"] + [b for b in P["biases"] if b is not None]
    opt = torch.optim.Adam(leaves, lr=1e-2, eps=1e-15)
    t_cpu = torch.from_numpy(target)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = ((G.forward(net, P, p, None, torch.float32)[0] - t_cpu) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    first, measure = losses[0], losses[-1]
    assert measure < first / 5, f"the measure does not train: {first:.4e} -> {measure:.4e}; re-seed"

    m = device_module(net)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, eps=1e-15)
    pos, t_dev = torch.from_numpy(p).to(DEV), t_cpu.to(DEV)
    for _ in range(steps):
        opt.zero_grad()
        ((m(pos) - t_dev) ** 2).mean().backward()
        opt.step()
    with torch.no_grad():
        final = float(((m(pos) - t_dev) ** 2).mean())
    note(f"it trains: initial loss {first:.6e}; after {steps} Adam steps the float32 CPU restatement {measure:.6e}, the module {final:.6e}")
    assert final <= 2 * measure


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pixie_amd import _lib, field_training as FT
    net, rows, p, extra, dY, keep, ref, yard, m_r = case("tcnn_F2_extra15")
    m = device_module(net)
    pos, ext = torch.from_numpy(p).to(DEV), torch.from_numpy(extra).to(DEV)
    with pytest.raises(ValueError, match="predict_normals"):
        m(pos.clone().requires_grad_(True), ext)
    with pytest.raises(_lib.PixieHipError):
        m(torch.from_numpy(p), torch.from_numpy(extra))
    with pytest.raises(_lib.PixieHipError):
        FT.TrainableHashMLP(None, None, [np.zeros((64, 3)), np.zeros((3, 64))], n_extra=3, device="cpu")
    out = m(pos, ext)
    out.sum().backward()
    with pytest.raises(RuntimeError):
        out.sum().backward()                                  # the saved arrays are gone: no second backward through the same graph
    e = ext.clone().requires_grad_(True)
    (ge,) = torch.autograd.grad((m(pos, e) ** 2).sum(), e, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        ge.sum().backward()                                   # no double backward
    for bad_pos, bad_ext in ((pos[:, :2], ext), (pos, ext[:, :3]), (pos, ext[:5]), (pos, None)):
        with pytest.raises(ValueError):
            m(bad_pos, bad_ext)
    lib = _lib.load()
    desc = m.to_hashmlp().desc()
    too_many = (1 << 24) + 1
    assert lib.pixie_hashmlp_forward_saved(C.byref(desc), None, None, too_many, None, None, None) != 0 and b"2^24" in lib.pixie_last_error()
    assert lib.pixie_hashmlp_backward(C.byref(desc), None, None, too_many, None, None, None, C.byref(_lib.HashMlpGrads()), None, None) != 0
    assert b"2^24" in lib.pixie_last_error()
    assert lib.pixie_hashmlp_train_bytes(C.byref(desc), too_many, None, None) != 0


def test_no_grad_saves_nothing_and_round_trips_share_storage():
    from pixie_amd import field_training as FT
    net, rows, p, extra, dY, keep, ref, yard, m_r = case("tcnn_F2_extra15")
    m = device_module(net)
    pos, ext = torch.from_numpy(p).to(DEV), torch.from_numpy(extra).to(DEV)
    with torch.no_grad():
        out = m(pos, ext)
    assert out.grad_fn is None and not out.requires_grad
    h = m.to_hashmlp()
    assert torch.equal(out, h(pos, ext))
    assert h.table.data_ptr() == m.table.data_ptr() and all(a.data_ptr() == b.data_ptr() for a, b in zip(h.weights, m.weights))
    back = FT.TrainableHashMLP.from_hashmlp(h)
    assert back.table.data_ptr() == h.table.data_ptr() and len(list(back.parameters())) == len(list(m.parameters()))
    for q in m.parameters():
        q.requires_grad_(False)
    assert m(pos, ext).grad_fn is None
    assert m(pos, ext.clone().requires_grad_(True)).grad_fn is not None


def test_feature_field_groups_and_query():
    from pixie_amd import field_query as FQ, field_training as FT
    rng = np.random.default_rng(3)
    fq = R.random_field(rng, "tcnn", 32)
    as_levels = lambda net: np.array([tuple(l[k] for k in FQ.LEVEL_DTYPE.names) for l in net["levels"]], FQ.LEVEL_DTYPE)
    part = lambda net: dict(levels=as_levels(net), table=net["table"], weights=net["weights"], biases=net["biases"], n_frequencies=net["n_frequencies"])
    field = FT.TrainableFeatureField.from_arrays(part(fq["density"]), dict(weights=fq["color"]["weights"], biases=fq["color"]["biases"]), part(fq["feature"]),
                                                 device=DEV)
    groups = field.get_param_groups()
    assert set(groups) == {"fields", "feature_field"}
    assert len(groups["fields"]) == len(list(field.density.parameters())) + len(list(field.color.parameters()))
    assert {id(q) for g in groups.values() for q in g} == {id(q) for q in field.parameters()}
    p = torch.from_numpy(rng.random((70, 3)).astype(np.float32)).to(DEV)
    out = field(p)
    (out["rgb"].sum() + out["feature"].sum() + out["density_out"][:, 0].sum()).backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in field.parameters())
    query = field.to_query()
    assert query.feature.table.data_ptr() == field.feature.table.data_ptr()
    feats, alphas, rgb = query.voxelize((-0.5,) * 3, (0.5,) * 3, 0.25)
    assert feats.shape[-1] == 32 and bool(torch.isfinite(feats.float()).all())
