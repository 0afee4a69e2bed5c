"""CPU pins of the 3DGS training-step natives' references (no device tensor is constructed here):

  * tests/_gs_optim_ref.py:densify_ref against tests/golden/gs_densify.npz, which the reference's own unmodified
    scene/gaussian_model.py wrote (tests/golden/make_gs_densify_golden.py): same row count and order, copied fields and moments
    bit-equal, computed fields (split xyz and scaling) to 1e-12 at float64;
  * the reference's optimiser surgery (gaussian_model.py:262-331, restated in _gs_optim_ref.py) against GaussianAdam's state
    layout, and state-dict exchange with torch.optim.Adam in both directions.
"""
import os

import numpy as np
import pytest
import torch

from tests import _gs_optim_ref as gr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gs_densify.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def before_of(golden, name):
    pre = f"{name}.before."
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre) and not k[len(pre):].startswith("step.")}


def test_golden_holds_every_case(golden):
    assert list(golden["cases"]) == list(gr.GOLDEN_CASES)
    for name, (n, degree, _, _) in gr.GOLDEN_CASES.items():
        assert golden[f"{name}.before.xyz"].shape == (n, 3) and n <= 128
        assert golden[f"{name}.before.f_rest"].shape == (n, (degree + 1) ** 2 - 1, 3)
        assert np.abs(golden[f"{name}.before.exp_avg.xyz"]).max() > 0            # the moments are those of a real step
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_mixed_population_has_every_kind(golden):
    """clone, split, pruned by opacity, pruned by world size, untouched, denom == 0, cloned-and-pruned -- and rows whose
    max_radii2D exceeds max_screen_size and that stay (the reference's dead prune term)"""
    b = before_of(golden, "mixed")
    ref = gr.densify_ref(b, gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, gr.MAX_SCREEN_SIZE, golden["mixed.z"])
    kept, clones, children, pruned = ref["counts"]
    assert kept > 0 and clones > 0 and children > 0 and pruned > 0 and ref["n_split"] > 0
    assert (b["denom"] == 0).any()
    src = ref["source_index"].numpy()
    n = b["xyz"].shape[0]
    prob = 1 / (1 + np.exp(-b["opacity"][:, 0].astype(np.float64)))
    smax = np.exp(b["scaling"].astype(np.float64)).max(axis=1)
    g = np.nan_to_num(b["xyz_gradient_accum"][:, 0].astype(np.float64) / np.where(b["denom"][:, 0] == 0, np.nan, b["denom"][:, 0]), nan=0.0)
    g = np.where((b["denom"][:, 0] == 0) & (b["xyz_gradient_accum"][:, 0] > 0), np.inf, g)
    cloned = (g >= gr.MAX_GRAD) & (smax <= gr.PERCENT_DENSE * gr.EXTENT)
    assert (cloned & (prob < gr.MIN_OPACITY)).any()                                # cloned and pruned
    assert ((g < gr.MAX_GRAD) & (smax > 0.1 * gr.EXTENT)).any()                    # pruned by world size alone
    assert ((g < gr.MAX_GRAD) & (prob < gr.MIN_OPACITY)).any()                     # pruned by opacity alone
    untouched = (g < gr.MAX_GRAD) & (prob >= gr.MIN_OPACITY) & (smax <= 0.1 * gr.EXTENT)
    assert untouched.any() and set(np.nonzero(untouched)[0]) <= set(src[:kept])
    assert (b["max_radii2D"][src[:kept]] > gr.MAX_SCREEN_SIZE).any()
    assert len(src) == kept + clones + children and src.max() < n


@pytest.mark.parametrize("name", list(gr.GOLDEN_CASES))
def test_restatement_matches_the_reference(golden, name):
    mss = gr.GOLDEN_CASES[name][2]
    b = before_of(golden, name)
    m = gr.margins(b)
    assert min(m.values()) > 1e-3, m
    z = golden[f"{name}.z"]
    r32 = gr.densify_ref(b, gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, mss, z, torch.float32)
    r64 = gr.densify_ref(b, gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, mss, z, torch.float64)
    assert r32["n_split"] == z.shape[0] // 2 and r32["counts"] == r64["counts"]
    m_rows = golden[f"{name}.after32.xyz"].shape[0]
    assert sum(r32["counts"][:3]) == m_rows
    n_old = r32["counts"][0] + r32["counts"][1]                  # rows whose every field is a copy
    for f in gr.FIELDS:
        want32, want64 = golden[f"{name}.after32.{f}"], golden[f"{name}.after64.{f}"]
        got32, got64 = r32[f].numpy(), r64[f].numpy()
        assert got32.shape == want32.shape and got64.shape == want64.shape, f
        if f in ("xyz", "scaling"):
            assert np.array_equal(got32[:n_old], want32[:n_old]), f
            assert np.array_equal(got64[:n_old], want64[:n_old]), f
            scale = max(1.0, float(np.abs(want64).max())) if want64.size else 1.0
            assert np.abs(got64 - want64).max(initial=0.0) <= 1e-12 * scale, f
            assert np.abs(got32 - want64).max(initial=0.0) <= 1e-5 * scale, f
        else:
            assert np.array_equal(got32, want32), f              # order and content: copies, bit for bit
            assert np.array_equal(got64, want64), f
        for mom in ("exp_avg.", "exp_avg_sq."):
            assert np.array_equal(r32[mom + f].numpy(), golden[f"{name}.after32.{mom}{f}"]), mom + f
            assert not r32[mom + f][r32["counts"][0]:].any(), mom + f
        assert golden[f"{name}.after32.step.{f}"] == golden[f"{name}.before.step.{f}"] == 1.0
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert np.array_equal(r32[k].numpy(), golden[f"{name}.after32.{k}"]), k
        assert not golden[f"{name}.after32.{k}"].any()
    # the source index reproduces every copied field from the state before
    src = r32["source_index"].numpy()
    assert np.array_equal(b["f_dc"][src], golden[f"{name}.after32.f_dc"])
    assert np.array_equal(b["rotation"][src], golden[f"{name}.after32.rotation"])


def test_stats_restatement_small_example():
    accum, denom, radii2d = torch.zeros(4, 1), torch.tensor([[0.0], [2.0], [0.0], [1.0]]), torch.tensor([0.0, 9.0, 2.0, 1.0])
    vgrad = torch.tensor([[3.0, 4.0, 7.0], [1.0, 0.0, 7.0], [6.0, 8.0, 7.0], [0.0, 0.0, 7.0]])
    radii = torch.tensor([5, 0, 1, 3], dtype=torch.int32)
    a, d, r = gr.stats_ref(accum, denom, radii2d, vgrad, radii)
    assert a.squeeze(1).tolist() == [5.0, 0.0, 10.0, 0.0]
    assert d.squeeze(1).tolist() == [1.0, 2.0, 1.0, 2.0]
    assert r.tolist() == [5.0, 9.0, 2.0, 3.0]


def _groups(n=6, degree=1):
    g = torch.Generator().manual_seed(3)
    k = (degree + 1) ** 2
    shapes = {"xyz": (n, 3), "f_dc": (n, 1, 3), "f_rest": (n, k - 1, 3), "opacity": (n, 1), "scaling": (n, 3), "rotation": (n, 4)}
    return [{"params": [torch.nn.Parameter(torch.randn(s, generator=g))], "lr": 1e-3 * (i + 1), "name": f} for i, (f, s) in enumerate(shapes.items())]


def _fill_state(opt, like):
    """the state layout after a step: GaussianAdam.init_state is what its step() creates"""
    for group in opt.param_groups:
        p = group["params"][0]
        st = like.init_state(p)
        st["step"] += 3
        st["exp_avg"] += 0.5
        st["exp_avg_sq"] += 0.25
        opt.state[p] = st


def test_reference_surgery_runs_on_gaussian_adam_state():
    from pixie_amd.gaussian_optim import GaussianAdam
    opt = GaussianAdam(_groups(), lr=0.0, eps=1e-15)
    assert isinstance(opt, torch.optim.Optimizer)
    assert [g["name"] for g in opt.param_groups] == list(gr.FIELDS) and opt.param_groups[0]["lr"] == 1e-3
    assert opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["eps"] == 1e-15
    # before any step there is no state, as with torch.optim.Adam: the reference's prune and cat take that branch
    assert gr.prune_optimizer(opt, torch.tensor([True, False, True, True, True, True]))["xyz"].shape == (5, 3)
    _fill_state(opt, GaussianAdam)
    ids = {g["name"]: id(opt.state[g["params"][0]]) for g in opt.param_groups}
    ext = {g["name"]: torch.ones((2,) + tuple(g["params"][0].shape[1:])) for g in opt.param_groups}
    new = gr.cat_tensors_to_optimizer(opt, ext)
    assert new["f_rest"].shape == (7, 3, 3) and opt.param_groups[2]["params"][0] is new["f_rest"]
    st = opt.state[new["xyz"]]
    assert st["exp_avg"].shape == (7, 3) and float(st["exp_avg"][:5].min()) == 0.5 and not st["exp_avg"][5:].any()
    mask = torch.tensor([True, True, False, True, False, True, True])
    new = gr.prune_optimizer(opt, mask)
    assert new["rotation"].shape == (5, 4) and opt.state[new["rotation"]]["exp_avg_sq"].shape == (5, 4)
    new = gr.replace_tensor_to_optimizer(opt, torch.full((5, 1), -4.0), "opacity")
    st = opt.state[new["opacity"]]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 3.0
    assert {g["name"]: id(opt.state[g["params"][0]]) for g in opt.param_groups} == ids      # the same dict objects throughout
    assert len(opt.state) == 6
    # update_learning_rate's access pattern
    for group in opt.param_groups:
        if group["name"] == "xyz":
            group["lr"] = 1.25e-4
    sd = opt.state_dict()
    assert sd["param_groups"][0]["lr"] == 1.25e-4 and sd["param_groups"][0]["name"] == "xyz"
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_state_dict_exchange_with_torch_adam():
    from pixie_amd.gaussian_optim import GaussianAdam
    ours = GaussianAdam(_groups(), lr=0.0, eps=1e-15)
    _fill_state(ours, GaussianAdam)
    theirs = torch.optim.Adam(_groups(), lr=0.0, eps=1e-15)
    theirs.load_state_dict(ours.state_dict())
    for group in theirs.param_groups:
        p = group["params"][0]
        p.grad = torch.ones_like(p)
    theirs.step()                                             # torch accepts the layout and keeps counting from our step
    p0 = theirs.param_groups[0]["params"][0]
    assert float(theirs.state[p0]["step"]) == 4.0 and theirs.param_groups[0]["name"] == "xyz"
    back = GaussianAdam(_groups(), lr=0.0, eps=1e-15)
    back.load_state_dict(theirs.state_dict())
    q0 = back.param_groups[0]["params"][0]
    assert float(back.state[q0]["step"]) == 4.0 and torch.equal(back.state[q0]["exp_avg"], theirs.state[p0]["exp_avg"])
    assert set(back.param_groups[0]) == set(theirs.param_groups[0])


def test_gaussian_adam_refusals_that_need_no_device():
    from pixie_amd.gaussian_optim import GaussianAdam
    p = lambda *s, **kw: torch.nn.Parameter(torch.zeros(*s, **kw))
    with pytest.raises(ValueError, match="weight decay"):
        GaussianAdam([{"params": [p(3, 3)], "name": "xyz"}], weight_decay=0.1)
    with pytest.raises(ValueError, match="amsgrad"):
        GaussianAdam([{"params": [p(3, 3)], "name": "xyz", "amsgrad": True}])
    with pytest.raises(ValueError, match="maximize"):
        GaussianAdam([{"params": [p(3, 3)], "name": "xyz"}], maximize=True)
    with pytest.raises(ValueError, match="exactly one tensor"):
        GaussianAdam([{"params": [p(3, 3), p(2)], "name": "xyz"}])
    with pytest.raises(ValueError, match="float32"):
        GaussianAdam([{"params": [p(3, 3, dtype=torch.float64)], "name": "xyz"}])
    with pytest.raises(ValueError, match="not contiguous"):
        GaussianAdam([{"params": [torch.nn.Parameter(torch.zeros(3, 4).t())], "name": "xyz"}])
    opt = GaussianAdam([{"params": [p(3, 3)], "name": "xyz"}])
    opt.param_groups[0]["params"][0].grad = torch.ones(3, 3)
    with pytest.raises(ValueError, match="host tensor"):
        opt.step()                                            # there is no CPU path
