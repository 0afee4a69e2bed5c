"""GaussianAdam (pixie_amd/gaussian_optim.py, one pixie_gs_adam_step launch per step) against torch.optim.Adam as
scene/gaussian_model.py:163 constructs it.

Oracle: torch.optim.Adam on the CPU at float64 from the same float32 inputs.  Yardstick y: the same optimiser on the CPU at
float32 against the float64 run.  For every group, for p, exp_avg and exp_avg_sq, after every step:
    max |HIP - float64| <= 3 y + 2 * 2^-24 * max |value|
(3: the project's margin; the floor is the last add's half-ulp on each side).

Sizes: N in {1, 5, 67, 1000} at SH degree 3 and at degree 0 (an empty f_rest group); N = 5 leaves a scalar tail in every group,
N = 67 crosses a wave.  Five steps per case: three with GaussianAdam, then one with a device torch.optim.Adam that loaded
GaussianAdam's state dict, then one with a fresh GaussianAdam that loaded torch's.  Learning rates differ per group and change
between steps.  Gradient magnitudes run from 1e-12 to 1e2 with random signs; in step 2 a third of the rows have exactly zero
gradients (invisible Gaussians).  v stays out of the float32 denormal range: the smallest gradient, 1e-12, gives
v = 0.001 * 1e-24 = 1e-27 after the first step, far above 1.2e-38, and a later zero gradient only scales it by 0.999.
The ratios to y are printed under -s (lines starting with "parity").
"""
import numpy as np
import pytest
import torch

from pixie_amd.gaussian_optim import FIELDS, GaussianAdam

pytestmark = pytest.mark.gpu

N_STEPS = 5
BASE_LR = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
LR_FACTOR = (1.0, 0.5, 2.0, 0.75, 1.5)
SIZES = [(n, d) for d in (3, 0) for n in (1, 5, 67, 1000)]


def shapes(n, degree):
    k = (degree + 1) ** 2
    return {"xyz": (n, 3), "f_dc": (n, 1, 3), "f_rest": (n, k - 1, 3), "opacity": (n, 1), "scaling": (n, 3), "rotation": (n, 4)}


def make_inputs(n, degree):
    rng = np.random.default_rng(1000 * n + degree)
    shp = shapes(n, degree)
    params = {f: rng.normal(0, 1, s).astype(np.float32) for f, s in shp.items()}
    grads = []
    for step in range(N_STEPS):
        g = {f: (rng.choice([-1.0, 1.0], s) * 10.0 ** rng.uniform(-12, 2, s)).astype(np.float32) for f, s in shp.items()}
        if step == 1:
            rows = rng.permutation(n)[:(n + 2) // 3]
            for f in g:
                g[f][rows] = 0.0
        grads.append(g)
    return params, grads


def groups_of(params, dtype, device):
    return [{"params": [torch.nn.Parameter(torch.from_numpy(params[f].copy()).to(device=device, dtype=dtype))], "lr": BASE_LR[f], "name": f}
            for f in FIELDS]


def one_step(opt, grads, step, dtype, device):
    for group in opt.param_groups:
        f = group["name"]
        group["lr"] = BASE_LR[f] * LR_FACTOR[step]
        group["params"][0].grad = torch.from_numpy(grads[step][f]).to(device=device, dtype=dtype)
    opt.step()
    snap = {}
    for group in opt.param_groups:
        p = group["params"][0]
        st = opt.state[p]
        snap[group["name"]] = tuple(t.detach().cpu().clone() for t in (p, st["exp_avg"], st["exp_avg_sq"]))
    return snap


def run_cpu(params, grads, dtype):
    opt = torch.optim.Adam(groups_of(params, dtype, "cpu"), lr=0.0, eps=1e-15)
    return [one_step(opt, grads, s, dtype, "cpu") for s in range(N_STEPS)]


def run_hip(params, grads, device):
    groups = groups_of(params, torch.float32, device)
    ours = GaussianAdam(groups, lr=0.0, eps=1e-15)
    snaps = [one_step(ours, grads, s, torch.float32, device) for s in range(3)]
    tensors = [g["params"][0] for g in ours.param_groups]
    regroup = lambda: [{"params": [p], "lr": BASE_LR[f], "name": f} for f, p in zip(FIELDS, tensors)]
    theirs = torch.optim.Adam(regroup(), lr=0.0, eps=1e-15)
    theirs.load_state_dict(ours.state_dict())
    snaps.append(one_step(theirs, grads, 3, torch.float32, device))
    back = GaussianAdam(regroup(), lr=0.0, eps=1e-15)
    back.load_state_dict(theirs.state_dict())
    snaps.append(one_step(back, grads, 4, torch.float32, device))
    assert float(back.state[tensors[0]]["step"]) == 5.0
    return snaps


_cache = {}


def reference(n, degree):
    """computed once per size and shared, never modified"""
    if (n, degree) not in _cache:
        params, grads = make_inputs(n, degree)
        _cache[(n, degree)] = (params, grads, run_cpu(params, grads, torch.float64), run_cpu(params, grads, torch.float32))
    return _cache[(n, degree)]


@pytest.mark.parametrize("n,degree", SIZES)
def test_three_steps_and_state_dict_round_trip_within_the_bar(hip_device, n, degree):
    params, grads, ref64, ref32 = reference(n, degree)
    hip = run_hip(params, grads, hip_device)
    worst = {"p": (0.0, 0.0), "exp_avg": (0.0, 0.0), "exp_avg_sq": (0.0, 0.0)}
    failures = []
    for step in range(N_STEPS):
        for f in FIELDS:
            for q, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
                want = ref64[step][f][q]
                if want.numel() == 0:
                    assert hip[step][f][q].numel() == 0
                    continue
                d = float((hip[step][f][q].double() - want).abs().max())
                y = float((ref32[step][f][q].double() - want).abs().max())
                bar = 3 * y + 2 * 2.0 ** -24 * float(want.abs().max())
                worst[name] = (max(worst[name][0], d / y if y > 0 else 0.0), max(worst[name][1], d / bar))
                if not d <= bar:
                    failures.append((step, f, name, d, y, bar))
    print(f"\nparity adam N={n} degree={degree}: max over 5 steps and 6 groups of d/y, d/bar: " +
          "; ".join(f"{k} {v[0]:.3f}, {v[1]:.3f}" for k, v in worst.items()))
    assert not failures, failures


@pytest.mark.parametrize("n,degree", [(67, 3), (5, 0)])
def test_bit_identical_from_run_to_run(hip_device, n, degree):
    params, grads, _, _ = reference(n, degree)
    a, b = run_hip(params, grads, hip_device), run_hip(params, grads, hip_device)
    for step in range(N_STEPS):
        for f in FIELDS:
            for q in range(3):
                assert torch.equal(a[step][f][q], b[step][f][q]), (step, f, q)


def test_zero_gradient_rows_still_move_on_their_momentum(hip_device):
    params, grads, ref64, _ = reference(67, 3)
    hip = run_hip(params, grads, hip_device)
    rows = np.nonzero((grads[1]["xyz"] == 0).all(axis=1))[0]
    assert len(rows) == 23
    moved = (hip[1]["xyz"][0][rows] != hip[0]["xyz"][0][rows])
    assert bool(moved.all())


def test_a_group_without_a_gradient_is_left_alone(hip_device):
    params, grads, _, _ = reference(5, 3)
    opt = GaussianAdam(groups_of(params, torch.float32, hip_device), lr=0.0, eps=1e-15)
    for group in opt.param_groups:
        if group["name"] != "scaling":
            group["params"][0].grad = torch.from_numpy(grads[0][group["name"]]).to(hip_device)
    opt.step()
    for group in opt.param_groups:
        p = group["params"][0]
        same = torch.equal(p.detach().cpu(), torch.from_numpy(params[group["name"]]))
        if group["name"] == "scaling":
            assert same and p not in opt.state
        else:
            assert not same and float(opt.state[p]["step"]) == 1.0


def test_refusals(hip_device):
    p = lambda *s, **kw: torch.nn.Parameter(torch.zeros(*s, device=hip_device, **kw))
    with pytest.raises(ValueError, match="weight decay"):
        GaussianAdam([{"params": [p(3, 3)], "name": "xyz", "weight_decay": 0.01}])
    with pytest.raises(ValueError, match="amsgrad"):
        GaussianAdam([{"params": [p(3, 3)], "name": "xyz"}], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        GaussianAdam([{"params": [p(3, 3)], "name": "xyz", "maximize": True}])
    with pytest.raises(ValueError, match="exactly one tensor"):
        GaussianAdam([{"params": [p(3, 3), p(2)], "name": "xyz"}])
    with pytest.raises(ValueError, match="float32"):
        GaussianAdam([{"params": [p(3, 3, dtype=torch.float16)], "name": "xyz"}])
    with pytest.raises(ValueError, match="not contiguous"):
        GaussianAdam([{"params": [torch.nn.Parameter(torch.zeros(3, 4, device=hip_device).t())], "name": "xyz"}])
    host = torch.nn.Parameter(torch.zeros(3, 3))
    opt = GaussianAdam([{"params": [host], "name": "xyz"}])
    host.grad = torch.ones(3, 3)
    with pytest.raises(ValueError, match="host tensor"):
        opt.step()
    assert not host.detach().any()
    # what the surgery can break after construction is refused by step() too
    opt = GaussianAdam([{"params": [p(3, 3)], "name": "xyz"}])
    opt.param_groups[0]["weight_decay"] = 0.5
    opt.param_groups[0]["params"][0].grad = torch.ones(3, 3, device=hip_device)
    with pytest.raises(ValueError, match="weight decay"):
        opt.step()
