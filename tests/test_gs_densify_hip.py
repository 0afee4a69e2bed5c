"""On-device densify_and_prune and the densification statistics (pixie_amd/gaussian_optim.py, pixie_amd/csrc/gs_optim.hip) against
the reference's own results (tests/golden/gs_densify.npz) and the torch restatement (tests/_gs_optim_ref.py).

Cases: the four golden ones; synthetic N in {1, 63, 257, 4099} (wave, workgroup and scan-block boundaries); all rows pruned (an
empty result), nothing cloned, nothing split.  Condition on the inputs, asserted on the CPU before a case is used: no quantity lies
within a relative 1e-3 of its threshold (g against max_grad, max(exp(scaling)) against percent_dense * extent and against
0.1 * extent, the split children's too, sigmoid(opacity) against min_opacity), so a device exp that differs by ulps cannot change
a decision.

Exact: the four counts, n_split, source_index, every copied field, every surviving moment; new moments zero; the statistics arrays
zero at the new length.  Computed (split scaling, split xyz): max |HIP - float64| <= 3 y + 4 * 2^-24 * max |value|, y being the
float32 restatement's distance from the float64 one for the same z.  The ratios are printed under -s (lines starting "parity").
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pixie_amd import _lib
from pixie_amd import gaussian_optim as go
from tests import _gs_optim_ref as gr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gs_densify.npz")
_cache = {}


def case_inputs(name):
    """(state before, z, max_screen_size, float32 reference, float64 reference): computed once, shared, never modified"""
    if name in _cache:
        return _cache[name]
    mss = gr.CASES[name][2]
    if name in gr.GOLDEN_CASES:
        if "golden" not in _cache:
            _cache["golden"] = dict(np.load(GOLDEN))
        gold = _cache["golden"]
        pre = f"{name}.before."
        state = {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre) and not k[len(pre):].startswith("step.")}
        z = gold[f"{name}.z"]
    else:
        state = gr.make_case(name)
        rng = np.random.default_rng(len(name))
        for f in gr.FIELDS:
            state["exp_avg." + f] = rng.normal(0, 1e-3, state[f].shape).astype(np.float32)
            state["exp_avg_sq." + f] = (rng.uniform(1e-8, 1e-4, state[f].shape)).astype(np.float32)
        z = state.pop("z")[:2 * gr.split_count(state)]
    m = gr.margins(state)
    assert min(m.values()) > 1e-3, (name, m)
    args = (gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, mss, z)
    _cache[name] = (state, z, mss, gr.densify_ref(state, *args, torch.float32), gr.densify_ref(state, *args, torch.float64))
    return _cache[name]


def run_hip(state, z, mss, device):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    params = {f: dev(state[f]) for f in gr.FIELDS}
    m = {f: dev(state["exp_avg." + f]) for f in gr.FIELDS}
    v = {f: dev(state["exp_avg_sq." + f]) for f in gr.FIELDS}
    return go.densify_and_prune_tensors(params, m, v, dev(state["xyz_gradient_accum"]), dev(state["denom"]), gr.MAX_GRAD, gr.MIN_OPACITY,
                                        gr.EXTENT, gr.PERCENT_DENSE, mss, noise=dev(z))


@pytest.mark.parametrize("name", list(gr.CASES))
def test_densify_and_prune_against_the_reference(hip_device, name):
    state, z, mss, r32, r64 = case_inputs(name)
    res = run_hip(state, z, mss, hip_device)
    counts = (res.n_kept, res.n_cloned, res.n_split_children, res.n_pruned)
    assert counts == r32["counts"] == r64["counts"] and res.n_split == r32["n_split"]
    m_rows = sum(counts[:3])
    if name == "all_pruned":
        assert m_rows == 0
    if name == "nothing_cloned":
        assert counts[1] == 0 and counts[2] > 0
    if name == "nothing_split":
        assert res.n_split == 0 and counts[1] > 0
    src = res.source_index.cpu().numpy()
    assert src.dtype == np.int32 and np.array_equal(src, r32["source_index"].numpy())
    n_old, n_kept = counts[0] + counts[1], counts[0]
    ratios = {}
    for f in gr.FIELDS:
        got = res.params[f].cpu().numpy()
        want = r32[f].numpy()
        assert got.shape == want.shape, f
        if f in ("xyz", "scaling"):
            assert np.array_equal(got[:n_old], want[:n_old]), f
            w64 = r64[f].numpy()[n_old:]
            if w64.size:
                d = np.abs(got[n_old:].astype(np.float64) - w64).max()
                y = np.abs(want[n_old:].astype(np.float64) - w64).max()
                bar = 3 * y + 4 * 2.0 ** -24 * np.abs(w64).max()
                ratios[f] = (d / y if y > 0 else 0.0, d / bar)
                assert d <= bar, (f, d, y, bar)
        else:
            assert np.array_equal(got, want), f
        for mom, out in (("exp_avg.", res.exp_avg), ("exp_avg_sq.", res.exp_avg_sq)):
            gm = out[f].cpu().numpy()
            assert gm.shape == want.shape
            assert np.array_equal(gm[:n_kept], state[mom + f][src[:n_kept]]), mom + f
            assert not gm[n_kept:].any(), mom + f
    if name in gr.GOLDEN_CASES:       # the reference's own output, not only the restatement of it
        gold = _cache["golden"]
        for f in ("f_dc", "f_rest", "opacity", "rotation"):
            assert np.array_equal(res.params[f].cpu().numpy(), gold[f"{name}.after32.{f}"]), f
        for f in gr.FIELDS:
            assert np.array_equal(res.exp_avg[f].cpu().numpy(), gold[f"{name}.after32.exp_avg.{f}"]), f
            assert np.array_equal(res.exp_avg_sq[f].cpu().numpy(), gold[f"{name}.after32.exp_avg_sq.{f}"]), f
    assert tuple(res.xyz_gradient_accum.shape) == (m_rows, 1) and tuple(res.denom.shape) == (m_rows, 1) and tuple(res.max_radii2D.shape) == (m_rows,)
    assert not res.xyz_gradient_accum.any() and not res.denom.any() and not res.max_radii2D.any()
    print(f"\nparity densify {name} N={state['xyz'].shape[0]} -> {m_rows} rows (split {res.n_split}): d/y, d/bar: " +
          ("; ".join(f"{k} {v[0]:.3f}, {v[1]:.3f}" for k, v in ratios.items()) or "no computed row"))


@pytest.mark.parametrize("n", [1, 67, 1000])
def test_statistics_kernel(hip_device, n):
    rng = np.random.default_rng(n)
    accum = rng.uniform(0, 1e-2, (n, 1)).astype(np.float32)
    denom = rng.integers(0, 50, (n, 1)).astype(np.float32)
    radii2d = rng.integers(0, 60, n).astype(np.float32)
    vgrad = (rng.normal(0, 1, (n, 3)) * 10.0 ** rng.uniform(-6, -2, (n, 1))).astype(np.float32)
    radii = rng.integers(-1, 80, n).astype(np.int32)
    radii[rng.permutation(n)[:n // 3]] = 0
    t = lambda a: torch.from_numpy(a.copy())
    a32, d32, r32 = gr.stats_ref(t(accum), t(denom), t(radii2d), t(vgrad), t(radii))
    a64, _, _ = gr.stats_ref(t(accum).double(), t(denom).double(), t(radii2d).double(), t(vgrad).double(), t(radii))
    da, dd, dr = (t(x).to(hip_device) for x in (accum, denom, radii2d))
    go.add_densification_stats(da, dd, dr, t(vgrad).to(hip_device), t(radii).to(hip_device))
    assert torch.equal(dd.cpu(), d32) and torch.equal(dr.cpu(), r32)
    got = da.cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(a64.numpy()).astype(np.float32)).astype(np.float64)
    err = np.abs(got - a64.numpy()) / ulp
    print(f"\nparity stats N={n}: accum max error {err.max():.3f} ulp (bar 2)")
    assert err.max() <= 2.0
    untouched = radii <= 0
    assert np.array_equal(da.cpu().numpy()[untouched], accum[untouched])


class StandIn:
    """the attributes of the reference's GaussianModel that the training step touches"""

    def __init__(self, state, device):
        p = lambda a: torch.nn.Parameter(torch.from_numpy(a.copy()).to(device))
        self._xyz, self._features_dc, self._features_rest = p(state["xyz"]), p(state["f_dc"]), p(state["f_rest"])
        self._opacity, self._scaling, self._rotation = p(state["opacity"]), p(state["scaling"]), p(state["rotation"])
        self.percent_dense = gr.PERCENT_DENSE
        self.xyz_gradient_accum = torch.from_numpy(state["xyz_gradient_accum"].copy()).to(device)
        self.denom = torch.from_numpy(state["denom"].copy()).to(device)
        self.max_radii2D = torch.from_numpy(state["max_radii2D"].copy()).to(device)
        lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-4, "scaling": 5e-5, "rotation": 1e-3}
        self.optimizer = go.GaussianAdam([{"params": [getattr(self, go._ATTR[f])], "lr": lrs[f], "name": f} for f in go.FIELDS], lr=0.0, eps=1e-15)

    def params(self):
        return [getattr(self, go._ATTR[f]) for f in go.FIELDS]

    def step(self, seed):
        g = torch.Generator().manual_seed(seed)
        for p in self.params():
            p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(p.device)
        self.optimizer.step()


def stand_in_run(device):
    state, z, mss, r32, _ = case_inputs("n257")
    gs = StandIn(state, device)
    gs.step(1)
    gs.step(2)
    # two Adam steps move scaling and opacity by at most 2 lr (1e-4 and 1e-3, relative to exp(scaling) and sigmoid(opacity)
    # too), and this case keeps every quantity 0.1 away from its threshold: the decisions are those of the state before
    assert min(gr.margins(state).values()) > 0.1
    noise = torch.from_numpy(z).to(device)
    res = go.densify_and_prune(gs, gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, mss, noise=noise)
    return gs, res, r32


def test_densify_and_prune_on_a_model_object(hip_device):
    gs, res, r32 = stand_in_run(hip_device)
    assert (res.n_kept, res.n_cloned, res.n_split_children, res.n_pruned) == r32["counts"]
    m_rows = res.n_kept + res.n_cloned + res.n_split_children
    assert np.array_equal(res.source_index.cpu().numpy(), r32["source_index"].numpy())
    for f, p in zip(go.FIELDS, gs.params()):
        group = [g for g in gs.optimizer.param_groups if g["name"] == f][0]
        assert group["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == m_rows
        st = gs.optimizer.state[p]
        assert float(st["step"]) == 2.0 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert not st["exp_avg"][res.n_kept:].any() and (st["exp_avg"][:res.n_kept].any() or p.numel() == 0)
    assert len(gs.optimizer.state) == 6
    assert gs.xyz_gradient_accum.shape == (m_rows, 1) and gs.denom.shape == (m_rows, 1) and gs.max_radii2D.shape == (m_rows,)
    before = gs._xyz.detach().clone()
    gs.step(3)                                      # the optimiser keeps stepping on the new tensors
    assert float(gs.optimizer.state[gs._xyz]["step"]) == 3.0 and not torch.equal(before, gs._xyz.detach())
    # statistics, then a second densify on the result (its own draw of the noise)
    radii = torch.arange(m_rows, dtype=torch.int32, device=hip_device) % 3
    go.add_densification_stats(gs.xyz_gradient_accum, gs.denom, gs.max_radii2D, torch.full((m_rows, 3), 1e-3, device=hip_device), radii)
    assert float(gs.denom.sum()) == float((radii > 0).sum())
    res2 = go.densify_and_prune(gs, gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, None, generator=torch.Generator(device=hip_device).manual_seed(5))
    m2 = res2.n_kept + res2.n_cloned + res2.n_split_children
    assert gs._xyz.shape == (m2, 3) and m2 > m_rows and res2.n_cloned + res2.n_split > 0
    assert bool(torch.isfinite(gs._xyz).all()) and float(gs.optimizer.state[gs._xyz]["step"]) == 3.0
    go.reset_opacity(gs)
    st = gs.optimizer.state[gs._opacity]
    assert float(torch.sigmoid(gs._opacity.detach()).max()) <= 0.01 * (1 + 1e-5) and not st["exp_avg"].any() and float(st["step"]) == 3.0
    gs.step(4)


def test_the_same_noise_gives_the_same_bits(hip_device):
    a, ra, _ = stand_in_run(hip_device)
    b, rb, _ = stand_in_run(hip_device)
    assert torch.equal(ra.source_index, rb.source_index)
    for pa, pb in zip(a.params(), b.params()):
        assert torch.equal(pa.detach(), pb.detach())
        assert torch.equal(a.optimizer.state[pa]["exp_avg_sq"], b.optimizer.state[pb]["exp_avg_sq"])


def test_refusals(hip_device):
    state, z, mss, _, _ = case_inputs("n63")
    for bad in (0.0, -1e-4):
        with pytest.raises(ValueError, match="max_grad"):
            dev = lambda a: torch.from_numpy(a.copy()).to(hip_device)
            go.densify_and_prune_tensors({f: dev(state[f]) for f in gr.FIELDS}, None, None, dev(state["xyz_gradient_accum"]), dev(state["denom"]),
                                         bad, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, mss)
    empty = {f: torch.zeros((0,) + state[f].shape[1:], device=hip_device) for f in gr.FIELDS}
    with pytest.raises(ValueError, match="no Gaussian"):
        go.densify_and_prune_tensors(empty, None, None, torch.zeros((0, 1), device=hip_device), torch.zeros((0, 1), device=hip_device),
                                     gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, mss)
    lib = _lib.load()
    desc = _lib.GsDensifyDesc()
    desc.n, desc.max_grad = 2 ** 31 - 1, 1e-4                 # refused before any pointer is looked at
    counts, n_split = (C.c_int64 * 4)(), (C.c_int64 * 1)()
    assert lib.pixie_gs_densify_plan(C.byref(desc), counts, n_split, None) == _lib.GS_DENSIFY_TOO_MANY_ROWS
    assert b"2^31 - 2" in lib.pixie_last_error()
    assert lib.pixie_gs_densify_workspace_bytes(2 ** 31 - 1) == -1
    with pytest.raises(ValueError, match="noise"):
        run_hip(state, z[:-1], mss, hip_device)               # the noise must have exactly 2 n_split rows
