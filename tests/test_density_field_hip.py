"""GPU checks of the proposal density field (pixie_amd.density_field, pixie_amd/csrc/density_field.hip) against the float64 torch
restatement of tests/_density_field_ref.py, whose gradients come from autograd.

Bar, for h and every gradient array: max |got - ref64| <= 3 x max |yardstick32 - ref64| + (sum of fan-ins + 16) 2^-24 max(1, max |ref64|)
(_hashmlp_grad_ref.bar), the yardstick being the same restatement in float32 on the CPU.  The table gradient gets m_r 2^-s more per
row: m_r contributions of at most 2^(-s-1) quantisation error each, s read back from the scratch header.  The density is held to the
bar on h times the density, plus 2 ulp.

ReLU kinks.  Points with a hidden unit whose float64 pre-activation is within float32's reach of zero (_hashmlp_grad_ref.undecided) get
their d_density zeroed on both sides; at most 2 % of a case's points may be zeroed, asserted from the reference alone.  (The float64
reference alone gives at most 0.15 % for these network shapes over seeds 0-3 at n = 2048.)

The measured ratios are appended to the file named by PIXIE_DENSITY_FIELD_PARITY_OUT when it is set (profiles/density_field_parity.txt
is such a run's output).
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import _density_field_ref as D
from tests import _field_query_ref as R
from tests import _hashmlp_grad_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 2048
CANARY = 123456.0

# name -> (convention, levels, base_res, max_res, log2_T, F, n_hidden, bias)
NETS = {
    "ns_5xF2": ("nerfstudio", 5, 16, 128, 12, 2, 1, True),
    "tcnn_5xF2_nobias": ("tcnn", 5, 16, 128, 12, 2, 1, False),      # level 0 is dense: 16^3 rows
    "ns_7xF2_h2": ("nerfstudio", 7, 16, 2048, 10, 2, 2, True),
    "tcnn_3xF4": ("tcnn", 3, 16, 64, 8, 4, 1, True),
    "linear": ("nerfstudio", 5, 16, 128, 12, 2, 0, True),
}
FRONTS = {
    "contraction": dict(contraction=True),
    "aabb": dict(contraction=False, aabb=[[-2.6, -2.7, -2.55], [2.65, 2.6, 2.6]]),      # about a third of [-3, 3]^3 falls outside
}
AID = 0.7
_cases = {}


def note(line):
    print(line)
    path = os.environ.get("PIXIE_DENSITY_FIELD_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def make_net(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    return D.random_net(rng, *NETS[name]), rng


def prepare(net, x, dD, front):
    bad = D.undecided(net, x, front)
    assert bad.mean() <= 0.02, f"{bad.mean():.4f} of the points sit on a ReLU kink"
    dD = dD.copy()
    dD[bad] = 0
    ref = D.evaluate(net, x, dD, torch.float64, front, AID)
    yard = D.evaluate(net, x, dD, torch.float32, front, AID)
    m_r = G.counts(net["levels"], ref["p"], ref["selector"] & ~bad, net["rows"])
    return dD, ref, yard, m_r


def case(name, front="contraction", n=N):
    key = (name, front, n)
    if key not in _cases:
        net, rng = make_net(name)
        x = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        dD = rng.standard_normal(n).astype(np.float32)
        _cases[key] = (net, x) + prepare(net, x, dD, FRONTS[front])
    return _cases[key]


def device_field(net, front, aid=AID):
    from pixie_amd import density_field as DF
    from pixie_amd import field_query as FQ
    f = DF.HashMLPDensityField.from_arrays(net["table"], net["weights"], net["biases"], aabb=front.get("aabb"),
                                           spatial_distortion=True if front.get("contraction", True) else None,
                                           implementation="torch" if net["convention"] == "nerfstudio" else "tcnn",
                                           world_to_nerf=front.get("world_to_nerf"), average_init_density=aid, device=DEV, **net["config"])
    want = np.array([tuple(l[k] for k in FQ.LEVEL_DTYPE.names) for l in net["levels"]], FQ.LEVEL_DTYPE)
    assert f.levels.tobytes() == want.tobytes(), "the module's level table is the restatement's"
    return f


def last_shift():
    from pixie_amd import density_field as DF
    head = DF._DensityFieldFunction.last_header.cpu().numpy().view(np.int32)
    return int(head[1]), int(head[2])


def device_eval(field, x, dD):
    field.zero_grad(set_to_none=True)
    density, raw = field(torch.from_numpy(x).to(DEV), return_raw=True)
    density[..., 0].backward(torch.from_numpy(dD).to(DEV))
    s, state = last_shift()
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return dict(h=host(raw)[:, 0], density=host(density)[:, 0], table=host(field.table.grad), weights=[host(w.grad) for w in field.weights],
                biases=[host(b.grad) if b is not None else None for b in field.bias_list()], s=s, state=state)


def arrays(g):
    yield "h", g["h"]
    yield "d_table", g["table"]
    for i, w in enumerate(g["weights"]):
        yield f"d_weight[{i}]", w
    for i, b in enumerate(g["biases"]):
        yield f"d_bias[{i}]", b


def within(got, ref, yard, net, m_r, what, scale=1.0, skip_h=False):
    """every array within `scale` x the bar (scale 2: two device implementations, each within its own)"""
    for (name, a), (_, r), (_, y) in zip(arrays(got), arrays(ref), arrays(yard)):
        if r is None or (skip_h and name == "h"):
            assert r is not None or a is None, name
            continue
        assert a is not None and a.shape == r.shape and np.all(np.isfinite(a)), f"{what} {name}"
        extra = m_r[:, None] * 2.0 ** -got["s"] if name == "d_table" else 0.0
        err = np.abs(a.astype(np.float64) - r)
        limit = scale * G.bar(r, y, [net], extra)
        yd = float(np.abs(y.astype(np.float64) - r).max())
        note(f"{what} {name}: max|got - f64| {err.max():.3e}, float32 CPU {yd:.3e} (ratio {err.max() / yd if yd else float('inf'):.2f}), "
             f"bar {float(np.min(limit)):.3e}" + (f", s {got['s']}" if name == "d_table" else ""))
        assert np.all(err <= limit), f"{what} {name}"


def density_within(got, ref, yard, net, what):
    h_bar = G.bar(ref["h"], yard["h"], [net])
    d = ref["density"]
    limit = h_bar * np.abs(d) + 2 * np.spacing(np.abs(d).astype(np.float32)).astype(np.float64)
    err = np.abs(got["density"].astype(np.float64) - d)
    note(f"{what} density: max err / limit {float(np.max(err / np.maximum(limit, 1e-300))):.3f} over {int((d != 0).sum())} points inside")
    assert np.all(err <= limit), what
    assert np.all(got["density"][~ref["selector"]] == 0), "selector 0 gives exactly 0"


# ---- 1. parity against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,front", [(n, "contraction") for n in sorted(NETS)] + [("ns_5xF2", "aabb")])
def test_parity(name, front):
    net, x, dD, ref, yard, m_r = case(name, front)
    inside = ref["selector"].mean()
    assert (front == "contraction" and inside == 1.0) or 0.55 < inside < 0.75, inside
    got = device_eval(device_field(net, FRONTS[front]), x, dD)
    assert got["state"] == 0
    within(got, ref, yard, net, m_r, f"parity {name} {front}")
    density_within(got, ref, yard, net, f"parity {name} {front}")


# ---- 2. tile edges, with canaries around every buffer the C API writes -----------------------------------------------------------------
def guarded(count):
    t = torch.full((count + 64,), CANARY, dtype=torch.float32, device=DEV)
    return t, t[32:32 + count]


def intact(whole, count):
    return bool((whole[:32] == CANARY).all() and (whole[32 + count:] == CANARY).all())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_tile_edges(n):
    from pixie_amd import _lib
    from pixie_amd import density_field as DF
    name = "ns_7xF2_h2"
    net, x, dD, ref, yard, m_r = case(name, "contraction", n)
    field = device_field(net, FRONTS["contraction"])
    desc = field.desc()
    pos, dd = torch.from_numpy(x).to(DEV), torch.from_numpy(dD).to(DEV)
    bufs = {"density": guarded(n), "raw": guarded(n), "table": guarded(field.table.numel())}
    for i, w in enumerate(field.weights):
        bufs[f"w{i}"] = guarded(w.numel())
        bufs[f"b{i}"] = guarded(w.shape[0])
    lib = _lib.load()
    ptr = lambda k: bufs[k][1].data_ptr()
    _lib.check(lib.pixie_density_field_forward(C.byref(desc), pos.data_ptr(), n, ptr("density"), ptr("raw"), None), "forward")
    g = _lib.DensityFieldGrads()
    g.d_table = ptr("table")
    for i in range(len(field.weights)):
        g.d_weight[i], g.d_bias[i] = ptr(f"w{i}"), ptr(f"b{i}")
    _, scratch_bytes = DF.train_bytes(desc, n)
    scratch_whole = torch.full((scratch_bytes + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    off = (-scratch_whole.data_ptr()) % 256
    _lib.check(lib.pixie_density_field_backward(C.byref(desc), pos.data_ptr(), n, dd.data_ptr(), C.byref(g), scratch_whole[off:].data_ptr(), None),
               "backward")
    torch.cuda.synchronize()
    for k, (whole, view) in bufs.items():
        assert intact(whole, view.numel()), f"n = {n}: canary around {k}"
    assert bool((scratch_whole[off + scratch_bytes:] == 0x5A).all()) and bool((scratch_whole[:off] == 0x5A).all()), "scratch overrun"
    head = scratch_whole[off:off + 12].cpu().numpy().view(np.int32)
    host = lambda k: bufs[k][1].cpu().numpy()
    got = dict(h=host("raw"), density=host("density"), table=host("table").reshape(field.table.shape),
               weights=[host(f"w{i}").reshape(w.shape) for i, w in enumerate(field.weights)], biases=[host(f"b{i}") for i in range(len(field.weights))],
               s=int(head[1]), state=int(head[2]))
    within(got, ref, yard, net, m_r, f"tile edge n = {n}")
    density_within(got, ref, yard, net, f"tile edge n = {n}")


# ---- 3. one point 1000 times: every atomic lands on the same 40 rows ---------------------------------------------------------------------
def test_one_point_a_thousand_times():
    name = "ns_5xF2"
    net, rng = make_net(name)
    x = np.tile(np.array([[0.3, -0.45, 0.61]], np.float32), (1000, 1))
    dD = rng.standard_normal(1000).astype(np.float32)
    front = FRONTS["contraction"]
    dD, ref, yard, m_r = prepare(net, x, dD, front)
    assert (ref["table"] != 0).any(axis=1).sum() <= 40 and m_r.max() >= 1000
    field = device_field(net, front)
    got = device_eval(field, x, dD)
    within(got, ref, yard, net, m_r, "one point x 1000")
    again = device_eval(field, x, dD)
    for (k, a), (_, b) in zip(arrays(got), arrays(again)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    assert np.all(got["density"].view(np.uint32) == got["density"].view(np.uint32)[0]), "the same point gets the same bits in every lane"


# ---- 4. runs and permutations --------------------------------------------------------------------------------------------------------
def bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("name", ["ns_5xF2", "ns_7xF2_h2"])
def test_runs_and_permutations(name):
    net, x, dD, ref, yard, m_r = case(name)
    field = device_field(net, FRONTS["contraction"])
    a, b = device_eval(field, x, dD), device_eval(field, x, dD)
    for (k, u), (_, v) in zip(arrays(a), arrays(b)):
        assert np.array_equal(bits(u), bits(v)), f"{k} differs from run to run"
    assert np.array_equal(bits(a["density"]), bits(b["density"]))
    perm = np.random.default_rng(3).permutation(len(x))
    c = device_eval(field, np.ascontiguousarray(x[perm]), np.ascontiguousarray(dD[perm]))
    assert np.array_equal(bits(c["density"]), bits(a["density"][perm])) and np.array_equal(bits(c["h"]), bits(a["h"][perm])), "densities under a permutation"
    assert np.array_equal(bits(c["table"]), bits(a["table"])) and c["s"] == a["s"], "the table gradient under a permutation"
    within(dict(c, h=a["h"]), ref, yard, net, m_r, f"permuted {name}")
    with torch.no_grad():
        for i in (0, 255, 256, 1000, N - 1):
            alone = field(torch.from_numpy(x[i:i + 1]).to(DEV)).cpu().numpy()
            assert bits(alone)[0, 0] == bits(a["density"])[i], f"point {i} alone"


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------
def test_selector_zero_points_get_nothing():
    net, _ = make_net("ns_5xF2")
    front = FRONTS["aabb"]
    lo, hi = np.asarray(front["aabb"], np.float32)
    nan = np.float32(np.nan)
    x = np.array([[lo[0], 0, 0], [0, hi[1], 0], [3, 0, 0], [0, 0, -2.9], lo, [nan, 0, 0], [0, nan, 0], [0, 0, nan], [np.inf, 0, 0]], np.float32)
    field = device_field(net, front)
    got = device_eval(field, x, np.ones(len(x), np.float32))
    assert np.all(bits(got["density"]) == 0), "density exactly +0"
    assert got["state"] == 1, "max |dX| == 0: no table atomic was issued"
    for k, a in arrays(got):
        if k != "h" and a is not None:
            assert np.all(a == 0), k
    assert np.all(np.isfinite(got["h"])) and np.all(bits(got["h"]) == bits(got["h"])[0]), "the raw output of a masked point is the network at p = 0"
    # the same points inside a batch: the batch's gradients are those of the batch with these points' upstream zeroed
    net, xb, dD, ref, yard, m_r = case("ns_5xF2", "aabb", 257)
    xb, dD2 = xb.copy(), dD.copy()
    xb[100:100 + len(x)] = x
    dD2[100:100 + len(x)] = 5.0
    a = device_eval(field, xb, dD2)
    dD2[100:100 + len(x)] = 0.0
    b = device_eval(field, xb, dD2)
    for (k, u), (_, v) in zip(arrays(a), arrays(b)):
        assert np.array_equal(bits(u), bits(v)), k
    contraction = device_eval(device_field(net, FRONTS["contraction"]), x[5:], np.ones(4, np.float32))
    assert np.all(bits(contraction["density"]) == 0) and contraction["state"] == 1, "NaN and Inf coordinates under contraction"


M_ONE = np.array([[1, 0.5, -0.25], [-1, 1, 1], [0.3, -1, 0.2], [1, 1, -1], [-0.25, 0.5, 1]], np.float32)


def test_m_exactly_one_takes_the_contraction_branch():
    """max |x| == 1 is not `m < 1`: the point goes through (2 - 1 / m) (x / m), as hashgrid_math.h does, and lands on (x + 2) / 4 with a
    coordinate at 0.25 or 0.75.  Such points sit in two waves of a batch: h, density and every gradient within the bar of float64
    with their upstream gradient non-zero, and their h and density bit-equal to the same point evaluated alone."""
    name, front, k = "ns_5xF2", FRONTS["contraction"], len(M_ONE)
    net, x, _, _, _, _ = case(name, "contraction", 257)
    x = x.copy()
    x[:k], x[70:70 + k] = M_ONE, M_ONE
    assert np.all(np.abs(x[:k]).max(axis=1) == 1)
    dD = np.random.default_rng(17).standard_normal(len(x)).astype(np.float32)
    dD, ref, yard, m_r = prepare(net, x, dD, front)
    assert np.all(dD[:k] != 0) and np.all(dD[70:70 + k] != 0), "the m == 1 points take part in the gradient check"
    assert ref["selector"][:k].all() and np.array_equal(bits(ref["p"][:k]), bits(((M_ONE + np.float32(2)) / np.float32(4)).astype(np.float32)))
    field = device_field(net, front)
    got = device_eval(field, x, dD)
    within(got, ref, yard, net, m_r, "m == 1 under contraction")
    density_within(got, ref, yard, net, "m == 1 under contraction")
    assert np.array_equal(bits(got["h"][:k]), bits(got["h"][70:70 + k])) and np.array_equal(bits(got["density"][:k]), bits(got["density"][70:70 + k]))
    without = dD.copy()
    without[:k], without[70:70 + k] = 0, 0
    assert not np.array_equal(device_eval(field, x, without)["table"], got["table"]), "they contribute to the table gradient"
    with torch.no_grad():
        for i in range(k):
            density, raw = field(torch.from_numpy(M_ONE[i:i + 1]).to(DEV), return_raw=True)
            assert bits(raw.cpu().numpy())[0, 0] == bits(got["h"])[i] and bits(density.cpu().numpy())[0, 0] == bits(got["density"])[i], f"point {i} alone"
            assert density[0, 0] > 0


def test_parameters_changed_in_place_before_the_backward_are_refused():
    """the backward recomputes the forward from the parameters' storage, so torch's version check must see them"""
    net, x, dD, _, _, _ = case("ns_5xF2", "contraction", 257)
    field = device_field(net, FRONTS["contraction"])
    out = field(torch.from_numpy(x).to(DEV))
    with torch.no_grad():
        field.table.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    out = field(torch.from_numpy(x).to(DEV))
    with torch.no_grad():
        field.bias_list()[0].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


@pytest.mark.parametrize("shift", [-20.0, 20.0, 100.0])
def test_trunc_exp_clamp(shift):
    """the output bias moved so that h ~ shift: the gradient follows exp(clamp(h, -15, 15)), h > 88 gives +Inf forward"""
    name = "ns_5xF2"
    net, x, dD, _, _, _ = case(name, "contraction", 257)
    net = dict(net, biases=net["biases"][:-1] + [np.array([shift], np.float32)])
    dD, ref, yard, m_r = prepare(net, x, dD, FRONTS["contraction"])
    with np.errstate(over="ignore"):
        got = device_eval(device_field(net, FRONTS["contraction"]), x, dD)
    assert abs(np.median(got["h"]) - shift) < 3
    within(got, ref, yard, net, m_r, f"clamp h ~ {shift}")
    scale = AID * np.exp(np.clip(ref["h"], -15, 15))
    want_db = float(np.sum(dD.astype(np.float64) * scale))
    assert abs(got["biases"][-1][0] - want_db) <= 1e-4 * np.sum(np.abs(dD) * scale), "d_bias_out = sum g exp(clamp(h)) average_init_density"
    if shift > 88:
        assert np.all(np.isposinf(got["density"])), "h > 88 gives +Inf"
    else:
        density_within(got, ref, yard, net, f"clamp h ~ {shift}")


def test_non_finite_upstream_and_refusals():
    from pixie_amd import _lib
    from pixie_amd import density_field as DF
    net, x, dD, _, _, _ = case("ns_5xF2", "contraction", 257)
    field = device_field(net, FRONTS["contraction"])
    bad = dD.copy()
    bad[7] = np.inf
    got = device_eval(field, x, bad)
    assert got["state"] == 2 and np.all(np.isnan(got["table"])), "a non-finite dX makes the whole table gradient NaN"
    pos = torch.from_numpy(x).to(DEV).requires_grad_(True)
    with pytest.raises(ValueError, match="positions get no gradient"):
        field(pos)
    with pytest.raises(_lib.PixieHipError):
        field(torch.from_numpy(x))
    with pytest.raises(ValueError, match="TrainableHashMLP"):
        DF.HashMLPDensityField(None, hidden_dim=64, spatial_distortion=True, device=DEV)
    with torch.no_grad():
        out = field(torch.from_numpy(x).to(DEV).reshape(1, 257, 3))
    assert out.shape == (1, 257, 1) and out.grad_fn is None
    rs = types.SimpleNamespace(frustums=types.SimpleNamespace(get_positions=lambda: torch.from_numpy(x).to(DEV).reshape(257, 1, 3)))
    density, nothing = field.get_density(rs)
    assert density.shape == (257, 1, 1) and nothing is None and density.grad_fn is not None
    assert np.array_equal(bits(density.detach().cpu().numpy().reshape(-1)), bits(out.cpu().numpy().reshape(-1))), "training and inference forwards agree"


# ---- 6. the zero-padded 64-wide twin -----------------------------------------------------------------------------------------------------
def torch_front_end(x, aid_sel=None):
    mag = x.abs().amax(dim=1, keepdim=True)
    p = torch.where(mag < 1, x, (2 - 1 / mag) * (x / mag))
    p = (p + 2.0) / 4.0
    sel = ((p > 0) & (p < 1)).all(dim=1)
    return p * sel[:, None], sel


@pytest.mark.parametrize("name", ["ns_5xF2", "tcnn_5xF2_nobias", "ns_7xF2_h2"])
def test_twin(name):
    """two device implementations, one answer: the fused 16-wide path against TrainableHashMLP on the zero-padded network with torch's
    contraction, selector and trunc_exp around it, each within its own bar of the float64 reference"""
    from pixie_amd import field_training as FT
    net, x, dD, ref, yard, m_r = case(name)
    field = device_field(net, FRONTS["contraction"])
    got = device_eval(field, x, dD)
    twin = field.to_trainable_hashmlp()
    xt = torch.from_numpy(x).to(DEV)
    p, sel = torch_front_end(xt)
    h = twin(p)[:, 0]
    density = AID * D.TruncExp.apply(h) * sel
    density.backward(torch.from_numpy(dD).to(DEV))
    s_twin = int(FT._HashMlpFunction.last_header.cpu().numpy().view(np.int32)[1])
    host = lambda t: t.detach().cpu().numpy()
    nh = len(net["weights"]) - 1
    tw = dict(h=host(h), density=host(density), table=host(twin.table.grad),
              weights=[host(w.grad)[:(16 if i < nh else 1), :(net["weights"][i].shape[1])] for i, w in enumerate(twin.weights)],
              biases=[host(b.grad)[:(16 if i < nh else 1)] if b is not None else None for i, b in enumerate(twin.bias_list())], s=s_twin)
    for i, w in enumerate(twin.weights):
        full = host(w.grad)
        assert np.all(full[(16 if i < nh else 1):] == 0), "the padding units are dead"
    for (k, a), (_, b), (_, r), (_, y) in zip(arrays(got), arrays(tw), arrays(ref), arrays(yard)):
        if r is None:
            continue
        extra = m_r[:, None] * (2.0 ** -got["s"] + 2.0 ** -tw["s"]) if k == "d_table" else 0.0
        limit = 2 * G.bar(r, y, [net]) + extra
        err = np.abs(a.astype(np.float64) - b.astype(np.float64))
        note(f"twin {name} {k}: max|16-wide - 64-wide| {err.max():.3e}, the sum of both bars {float(np.min(limit)):.3e}")
        assert np.all(err <= limit), k
    within(tw, ref, yard, net, m_r, f"twin {name} (64-wide)")


# ---- 7. inside the sampler -------------------------------------------------------------------------------------------------------------
def test_inside_the_proposal_sampler():
    from pixie_amd import density_field as DF
    from pixie_amd import ray_sampling as rs
    from tests import _ray_sampling_ref as ref
    bundle = ref.make_bundle(32, seed=4)
    bundle = types.SimpleNamespace(**{k: v.to(DEV) for k, v in vars(bundle).items()})

    def run():
        torch.manual_seed(11)
        fields = [DF.HashMLPDensityField(None, spatial_distortion=True, num_levels=5, max_res=m, base_res=16, log2_hashmap_size=12,
                                         implementation="torch", device=DEV) for m in (128, 256)]
        with torch.no_grad():
            for f in fields:
                f.table.mul_(300.0)                        # the reference's 1e-3 initialisation gives a near-constant density
        sampler = rs.ProposalNetworkSampler(num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=4, single_jitter=True)
        samples, weights_list, samples_list = sampler(bundle, [f.density_fn for f in fields])
        # fine weights with all their mass in one interval per ray: no smooth proposal histogram bounds them, so the loss is positive
        fine = torch.zeros(32, 4, 1, device=DEV)
        fine[torch.arange(32), torch.arange(32) % 4] = 0.9
        loss = rs.interlevel_loss(weights_list + [fine], samples_list + [samples])
        assert float(loss.detach()) > 0
        loss.backward()
        return fields, sampler, float(loss.detach()), [p.grad.detach().cpu().numpy() for f in fields for p in f.parameters()]

    fields, sampler, loss, grads = run()
    assert np.isfinite(loss)
    for g in grads:
        assert np.all(np.isfinite(g)) and np.any(g != 0)
    _, _, loss2, grads2 = run()
    assert loss == loss2 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(grads, grads2)), "a seeded run is bit-identical twice"
    sampler.update_sched = lambda step: 5
    sampler.step_cb(20)
    _, weights_list, _ = sampler(bundle, [f.density_fn for f in fields])
    assert all(w.grad_fn is None and not w.requires_grad for w in weights_list), "updated false: the densities carry no grad_fn"


# ---- 8. it trains ------------------------------------------------------------------------------------------------------------------------
def target_density(x):
    return 4.0 * torch.exp(-3.0 * (x * x).sum(dim=1)) + 0.2


def cpu_training(net, x, steps, lr, order=None):
    """the float32 restatement under torch.optim.Adam, the points taken in `order`"""
    x = x if order is None else np.ascontiguousarray(x[order])
    masked, sel = D.front_end(x, FRONTS["contraction"])
    P = G.params(net, torch.float32)
    leaves = [P["table"]] + P["weights"] + [b for b in P["biases"] if b is not None]
    opt = torch.optim.Adam(leaves, lr=lr)
    want = target_density(torch.from_numpy(x))
    s = torch.from_numpy(sel.astype(np.float32))
    for step in range(steps + 1):
        opt.zero_grad()
        h = G.forward(net, P, masked, None, torch.float32)[0]
        loss = ((D.TruncExp.apply(h[:, 0]) * s - want) ** 2).mean()
        if step < steps:
            loss.backward()
            opt.step()
    return float(loss.detach())


def test_it_trains():
    """150 Adam steps on a smooth analytic density, n = 1024, the 3-level net; the final loss against the float32 CPU restatement from
    the same initial values.  Tolerance: 3 x the restatement's own spread (max - min of its final loss) over three permutations of
    the points.  (Measured: loss 0.4886 -> 0.001923 on both sides; spread 4.7e-10, |device - CPU| 3.5e-10: a few ulps of the loss.)"""
    steps, lr, n = 150, 1e-2, 1024
    net, rng = make_net("tcnn_3xF4")
    net = dict(net, table=(0.1 * net["table"]).astype(np.float32))
    x = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    base = cpu_training(net, x, steps, lr)
    perms = [cpu_training(net, x, steps, lr, np.random.default_rng(100 + k).permutation(n)) for k in range(3)]
    spread = max(perms) - min(perms)
    field = device_field(net, FRONTS["contraction"], aid=1.0)
    opt = torch.optim.Adam(field.parameters(), lr=lr)
    xt = torch.from_numpy(x).to(DEV)
    want = target_density(xt)
    first = None
    for step in range(steps + 1):
        opt.zero_grad()
        loss = ((field(xt)[:, 0] - want) ** 2).mean()
        first = float(loss.detach()) if first is None else first
        if step < steps:
            loss.backward()
            opt.step()
    final = float(loss.detach())
    note(f"training: loss {first:.6f} -> {final:.6f} on the device, {base:.6f} on the CPU in float32; permutations of the CPU run "
         f"{', '.join(f'{p:.6f}' for p in perms)} (spread {spread:.3e}); |device - CPU| {abs(final - base):.3e}, tolerance {3 * spread:.3e}")
    assert final < 0.5 * first, "it trains"
    assert abs(final - base) <= 3 * spread


# ---- 9. state dicts ----------------------------------------------------------------------------------------------------------------------
def test_state_dict_constructors():
    from pixie_amd import density_field as DF
    rng = np.random.default_rng(9)
    cfg = dict(aabb=None, spatial_distortion=True, num_layers=2, hidden_dim=16, num_levels=5, max_res=128, base_res=16, log2_hashmap_size=12,
               features_per_level=2, device=DEV)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    # nerfstudio's torch implementation: Sequential(HashEncoding, MLP) under mlp_base
    sd = {"prop.0.mlp_base.0.hash_table": torch.from_numpy(f32(5 << 12, 2)), "prop.0.mlp_base.1.layers.0.weight": torch.from_numpy(f32(16, 10)),
          "prop.0.mlp_base.1.layers.0.bias": torch.from_numpy(f32(16)), "prop.0.mlp_base.1.layers.1.weight": torch.from_numpy(f32(1, 16)),
          "prop.0.mlp_base.1.layers.1.bias": torch.from_numpy(f32(1))}
    f = DF.HashMLPDensityField.from_nerfstudio_state_dict(sd, "prop.0", cfg)
    assert f.implementation == "torch" and f.n_hidden == 1 and len(f.biases) == 2
    assert torch.equal(f.table.detach().cpu(), sd["prop.0.mlp_base.0.hash_table"]) and torch.equal(f.weights[1].detach().cpu(), sd["prop.0.mlp_base.1.layers.1.weight"])
    assert torch.equal(f.bias_list()[0].detach().cpu(), sd["prop.0.mlp_base.1.layers.0.bias"])
    lin = {"p.mlp_base.0.hash_table": sd["prop.0.mlp_base.0.hash_table"], "p.linear.weight": torch.from_numpy(f32(1, 10)), "p.linear.bias": torch.from_numpy(f32(1))}
    g = DF.HashMLPDensityField.from_nerfstudio_state_dict(lin, "p", dict(cfg, use_linear=True))
    assert g.n_hidden == 0 and torch.equal(g.weights[0].detach().cpu(), lin["p.linear.weight"])
    with pytest.raises(ValueError, match="hash table"):
        DF.HashMLPDensityField.from_nerfstudio_state_dict(dict(sd, **{"prop.0.mlp_base.0.hash_table": torch.zeros(100, 2)}), "prop.0", cfg)
    # tiny-cuda-nn: the grid's vector and the 16-wide FullyFusedMLP's: (16, 16) [10 inputs padded to 16] then (16, 16) [1 output padded]
    t = DF.HashMLPDensityField(**dict(cfg, implementation="tcnn"))
    rows = t.table.shape[0]
    enc, mlp = f32(rows * 2), f32(16 * 16 + 16 * 16)
    t = DF.HashMLPDensityField.from_tcnn_params(enc, mlp, cfg)
    assert t.implementation == "tcnn" and np.array_equal(t.table.detach().cpu().numpy().reshape(-1), enc)
    w0 = mlp[:256].reshape(16, 16)
    assert np.array_equal(t.weights[0].detach().cpu().numpy(), w0[:, :10]) and np.array_equal(t.weights[1].detach().cpu().numpy(), mlp[256:].reshape(16, 16)[:1])
    assert np.allclose(t.bias_list()[0].detach().cpu().numpy(), w0[:, 10:].sum(axis=1), atol=1e-5) and t.bias_list()[1] is None
    with pytest.raises(ValueError, match="params holds"):
        DF.HashMLPDensityField.from_tcnn_params(enc, mlp[:-1], cfg)
    with pytest.raises(ValueError, match="encoding_params holds"):
        DF.HashMLPDensityField.from_tcnn_params(enc[:-2], mlp, cfg)
    # the parameters ARE the descriptor's storage, across an optimiser step
    ptrs = [p.data_ptr() for p in f.parameters()]
    d = f.desc()
    assert d.d_table == f.table.data_ptr() and d.d_weight[0] == f.weights[0].data_ptr() and d.d_bias[1] == f.bias_list()[1].data_ptr()
    opt = torch.optim.SGD(f.parameters(), lr=0.1)
    x = torch.from_numpy(rng.uniform(-1, 1, (300, 3)).astype(np.float32)).to(DEV)
    before = f(x).detach().clone()
    f(x).sum().backward()
    opt.step()
    assert [p.data_ptr() for p in f.parameters()] == ptrs and f.desc().d_table == d.d_table
    assert not torch.equal(f(x).detach(), before), "the next launch reads the stepped parameters"
    assert set(dict(f.named_parameters())) == {"table", "weights.0", "weights.1", "biases.0", "biases.1"}
