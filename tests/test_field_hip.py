"""GPU parity tests of the field -> particle transfer (csrc/field_transfer.hip through pixie_amd.material_field, i.e. the
C ABI) against the golden vectors produced by the reference's own code and against oracle/field_oracle.py.
Integer outputs (material id, part label, too-far set) bit-exact; float32 outputs within 2e-6 relative (powf and the
float64 defaults differ from numpy in the last ulp), distances 1e-6."""
import os

import numpy as np
import pytest
import torch

from oracle import field_oracle
from tests._field_parity import compare

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "field_transfer.npz")


def run_hip(dev, pred, mask, lo, hi, pos, **kw):
    from pixie_amd.material_field import field_to_particles
    out = field_to_particles(torch.from_numpy(pred).to(dev), torch.from_numpy(mask).to(dev), lo, hi, torch.from_numpy(pos).to(dev), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("weighted", [False, True])
def test_matches_reference_golden(hip_device, weighted):
    g = np.load(GOLD)
    got = run_hip(hip_device, g["pred"], g["mask"], g["min_bounds"], g["max_bounds"], g["particle_pos"], k=10,
                  nn_distance_threshold=0.1, weighted=weighted)
    tag = "w_" if weighted else "u_"
    ref = {k: g[tag + k] for k in ("material_id", "part_labels", "density", "E", "nu", "conf", "nearest_dist")}
    compare(got, ref, g[tag + "too_far"])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D,n,k", [(32, 20000, 10), (16, 500, 1), (20, 3000, 16)])
def test_matches_oracle_on_other_shapes(hip_device, D, n, k, weighted):
    rng = np.random.default_rng(D + n)
    pred = rng.normal(0, 0.6, size=(11, D, D + 2, D - 3)).astype(np.float32)
    mask = (rng.random((D, D + 2, D - 3)) < 0.5).astype(np.float32)       # sparse, anisotropic lattice
    lo, hi = np.array([0.0, -1.0, 2.0]), np.array([1.5, 1.0, 3.0])
    pos = (lo + (hi - lo) * rng.random((n, 3)) * 1.1 - 0.05 * (hi - lo)).astype(np.float32)  # some outside the lattice
    got = run_hip(hip_device, pred, mask, lo, hi, pos, k=k, nn_distance_threshold=0.08, weighted=weighted)
    ref = field_oracle.field_to_particles(pred, mask, lo, hi, pos, k=k, nn_distance_threshold=0.08, weighted=weighted)
    compare(got, ref, ref["too_far"])


def test_full_size_and_solver_handoff(hip_device):
    """BASELINE size: a 128^3 field (18 % occupied ball) onto 100k particles; the result feeds MPM_Simulator_WARP.
    Size-independent properties: every assigned value lies in the hull of the un-scaled field, ids are valid classes,
    particles inside the ball are all assigned."""
    from pixie_amd.material_field import NORMALIZATION_RANGES as R, apply_material_field_to_solver, field_to_particles
    from pixie_amd.mpm_solver import MPM_Simulator_WARP
    D, n = 128, 100_000
    gen = torch.Generator(device="cpu").manual_seed(0)
    pred = torch.zeros((11, D, D, D))
    pred[:3] = torch.randn((3, D, D, D), generator=gen) * 0.5
    cls = torch.randint(0, 8, (D, D, D), generator=gen)
    pred[3:] = torch.nn.functional.one_hot(cls, 8).permute(3, 0, 1, 2).float()
    g = (torch.arange(D) - (D - 1) / 2) / (D / 2)
    rr = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2).sqrt()
    mask = (rr < 0.7).float()
    d = torch.randn((n, 3), generator=gen); d = d / d.norm(dim=1, keepdim=True)
    pos = d * (0.6 * torch.rand(n, generator=gen) ** (1 / 3))[:, None]
    out = field_to_particles(pred.to(hip_device), mask.to(hip_device), [-1, -1, -1], [1, 1, 1], pos.to(hip_device))
    assert int(out["n_too_far"]) == 0
    dens = out["density"].cpu()
    assert float(dens.min()) >= 10 ** R["density_min"] * (1 - 1e-5) and float(dens.max()) <= 10 ** R["density_max"] * (1 + 1e-5)
    nu = out["nu"].cpu()
    assert float(nu.min()) >= R["nu_min"] - 1e-6 and float(nu.max()) <= R["nu_max"] + 1e-6
    mid = out["material_id"].cpu()
    assert int(mid.min()) >= 0 and int(mid.max()) <= 7 and torch.equal(mid, out["part_labels"].cpu())
    assert float(out["conf"].min()) == 1.0   # one-hot scores
    s = MPM_Simulator_WARP(10)
    s.load_initial_data_from_torch(pos + 1.0, torch.full((n,), 1e-6), n_grid=50, grid_lim=2.0)
    s.set_parameters_dict(dict(material="jelly", E=1e5, nu=0.3, density=1000.0))
    conf = apply_material_field_to_solver(s, pred.to(hip_device), mask.to(hip_device), [-1, -1, -1], [1, 1, 1], pos.to(hip_device))
    assert conf.shape == (n,)
    assert torch.allclose(s.get_field("E").cpu(), out["E"].cpu()) and torch.equal(s.get_field("material").cpu(), mid)


def test_empty_and_nearly_empty_masks(hip_device):
    """Edge of the field -> particle transfer: a mask that keeps no voxel, or fewer than k.  sklearn's NearestNeighbors -- the reference's
    perform_knn_smoothing, material_field.py:228-300 -- raises there; the host-level entry raises the same ValueError, and the device-resident
    entry hands every particle the defaults (n_too_far = n) WITHOUT walking the lattice once per particle (a 128^3 field and 100 k
    particles: this test would not finish otherwise)."""
    import time
    from pixie_amd.material_field import apply_material_field_to_solver, field_to_particles
    from pixie_amd.mpm_solver import MPM_Simulator_WARP
    D, n = 128, 100_000
    gen = torch.Generator().manual_seed(3)
    pred = torch.zeros((11, D, D, D))
    pred[:3] = torch.randn((3, D, D, D), generator=gen) * 0.5
    pred[3] = 1.0
    pos = (torch.rand((n, 3), generator=gen) - 0.5)
    for kept in (0, 4):
        mask = torch.zeros((D, D, D))
        mask.view(-1)[torch.randperm(D ** 3, generator=gen)[:kept]] = 1.0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = field_to_particles(pred.to(hip_device), mask.to(hip_device), [-1, -1, -1], [1, 1, 1], pos.to(hip_device), k=10)
        assert int(out["n_too_far"]) == n and int(out["n_occupied_voxels"]) == kept
        assert time.perf_counter() - t0 < 5.0
        for key in ("density", "E", "nu", "conf"):
            assert torch.isfinite(out[key]).all()
        assert int(out["material_id"].min()) == int(out["material_id"].max())      # the default material for everyone
        s = MPM_Simulator_WARP(10)
        s.load_initial_data_from_torch(pos + 1.0, torch.full((n,), 1e-6), n_grid=50, grid_lim=2.0)
        s.set_parameters_dict(dict(material="jelly", E=1e5, nu=0.3, density=1000.0))
        with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
            apply_material_field_to_solver(s, pred.to(hip_device), mask.to(hip_device), [-1, -1, -1], [1, 1, 1], pos.to(hip_device))
