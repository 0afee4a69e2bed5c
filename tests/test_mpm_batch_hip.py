"""GPU tests of the fused multi-scene MPM step (pixie_amd.mpm_solver.SceneBatch, C ABI pixie_mpm_batch_*): every scene of a batch
must end in exactly the bits it reaches when it is stepped alone with run() -- particle state, time, re-binning count, lost-particle
counters and the exported grid."""
import numpy as np
import pytest
import torch

from pixie_amd import _lib
from pixie_amd.synthetic import apply_scene, mpm_ball_scene, mpm_plastic_scene

pytestmark = pytest.mark.gpu

DT = 1e-4
FIELDS = ("x", "v", "C", "F", "F_trial", "stress", "selection", "grid_v_out")


def make(scene, setup=None):
    from pixie_amd.mpm_solver import MPM_Simulator_WARP
    s = MPM_Simulator_WARP(10)
    s.load_initial_data_from_torch(torch.from_numpy(scene["x"]), torch.from_numpy(scene["vol"]), torch.from_numpy(scene["cov"]),
                                   n_grid=scene["n_grid"], grid_lim=scene["grid_lim"])
    apply_scene(s, scene, per_particle=scene.get("per_particle", True))
    for name in ("F_trial", "v"):
        key = {"F_trial": "F0", "v": "v0"}[name]
        if key in scene:
            s.set_field(name, torch.from_numpy(np.ascontiguousarray(scene[key].reshape(scene[key].shape[0], -1))))
    if setup:
        setup(s)
    return s


def pair(scene, setup=None):
    return make(scene, setup), make(scene, setup)


def assert_same(b, a, tag=""):
    for f in FIELDS:
        assert torch.equal(b.get_field(f), a.get_field(f)), f"{tag}: {f}"
    assert b.time == a.time, tag
    for k in ("n_rebins", "slow_path_particles", "dropped_particles", "lost_particles_seen", "item_cap", "scatter_bits"):
        assert b._get_scalar(k) == a._get_scalar(k), f"{tag}: {k}"
    assert b.out_of_bounds == a.out_of_bounds, tag


def heterogeneous_scenes():
    """jelly tree (impulse that opens and closes inside the first call, ground slab), jelly ball (bounding box), sand on a sticky
    floor, snow column under a moving cuboid"""
    tree = mpm_ball_scene(5_000, seed=1, n_grid=32, scenario="tree")
    tree["bcs"] = [dict(type="particle_impulse", force=[-0.48, 0.0, 0.1], num_dt=5, start_time=10 * DT)]
    ball = mpm_ball_scene(30_000, seed=2, n_grid=48, scenario="ball")
    sand = mpm_ball_scene(100_000, seed=3, n_grid=64, scenario="sand")
    sand["per_particle"] = False
    snow = mpm_plastic_scene("snow", 20_000, seed=4)
    snow["n_grid"], snow["dt"] = 40, DT
    snow["x"] = (1.0 + (snow["x"] - 1.0) * np.array([0.4, 0.4, 1.0], np.float32)).astype(np.float32)   # a column
    snow["bcs"] = [dict(type="bounding_box"),
                   dict(type="cuboid", point=[1.0, 1.0, 0.55], size=[0.3, 0.3, 0.05], velocity=[0.0, 0.2, 0.1], start_time=0.0,
                        end_time=6e-3, reset=1)]
    return [tree, ball, sand, snow]


def test_heterogeneous_batch_equals_solo_runs(hip_device):
    from pixie_amd.mpm_solver import SceneBatch
    scs = heterogeneous_scenes()
    batch, alone = zip(*[pair(sc) for sc in scs])
    rebins = []
    with SceneBatch(batch) as sb:
        for call in range(3):
            sb.run(DT, 40)
            for a in alone:
                a.run(DT, 40)
            rebins.append([int(b._get_scalar("n_rebins")) for b in batch])
            for i, (b, a) in enumerate(zip(batch, alone)):
                assert_same(b, a, f"call {call} scene {i}")
    print("re-binnings per scene after each call:", rebins)
    assert len({tuple(r) for r in zip(*rebins)}) > 1      # the scenes re-bin on their own cadences
    for b in batch:
        assert np.isfinite(b.get_field("x").cpu().numpy()).all()


def test_variant_grouping(hip_device):
    """scenes that need different kernel variants in one batch: scatter mode 64 next to 32, and 256-thread work items (dense) next to
    128-thread ones (sparse) -- one launch per group, bit-identical to solo"""
    from pixie_amd.mpm_solver import SceneBatch
    scs = [mpm_ball_scene(30_000, seed=10, n_grid=48, scenario="ball"), mpm_ball_scene(30_000, seed=11, n_grid=48, scenario="tree"),
           mpm_ball_scene(100_000, seed=12, n_grid=50, scenario="ball"), mpm_ball_scene(100_000, seed=13, n_grid=160, scenario="ball")]
    setups = [lambda s: s._set_scalar("scatter_bits", 64), lambda s: s._set_scalar("scatter_bits", 32), None, None]
    batch, alone = zip(*[pair(sc, st) for sc, st in zip(scs, setups)])
    with SceneBatch(batch) as sb:
        for call in range(2):
            sb.run(DT, 30)
            for a in alone:
                a.run(DT, 30)
            for i, (b, a) in enumerate(zip(batch, alone)):
                assert_same(b, a, f"call {call} scene {i}")
    assert [int(b._get_scalar("scatter_bits")) for b in batch[:2]] == [64, 32]
    assert int(batch[2]._get_scalar("item_cap")) == 256 and int(batch[3]._get_scalar("item_cap")) == 128


def test_every_fused_variant_batched_equals_solo(hip_device):
    """one scene per fused kernel variant -- wide + packed scatter, five waves + packed, wide + exact, six waves (exact only) -- in one
    batch: the solo and the batched launch read one variant table (dispatch_block_variant), and the variants round differently, so a
    scene that got another kernel in the batch would differ from its solo run"""
    from pixie_amd.mpm_solver import SceneBatch
    scs = [mpm_ball_scene(5_000, seed=70 + i, n_grid=32) for i in range(4)]
    settings = [dict(wide=1), dict(wide=0), dict(wide=1, scatter_bits=64), dict(occupancy=6, scatter_bits=64, wide=0)]
    setups = [lambda s, kv=kv: [s._set_scalar(k, v) for k, v in kv.items()] for kv in settings]
    batch, alone = zip(*[pair(sc, st) for sc, st in zip(scs, setups)])
    with SceneBatch(batch) as sb:
        sb.run(DT, 30)
        for i, (b, a) in enumerate(zip(batch, alone)):
            a.run(DT, 30)
            assert_same(b, a, f"scene {i} {settings[i]}")
    assert [int(b._get_scalar("scatter_bits")) for b in batch] == [32, 32, 64, 64]


def test_batch_of_one_equals_pixie_mpm_step(hip_device):
    from pixie_amd.mpm_solver import SceneBatch
    sc = mpm_ball_scene(30_000, seed=20, n_grid=40, scenario="tree")
    b, a = pair(sc)
    with SceneBatch([b]) as sb:
        sb.run(DT, 0)                 # a no-op
        assert b.time == 0.0 and int(b._get_scalar("n_rebins")) == 0
        sb.run(DT, 50)
        sb.run(DT, 7)
    a.run(DT, 50)
    a.run(DT, 7)
    assert_same(b, a)


def test_ordering_after_deferred_substeps(hip_device):
    """a deferred p2g2p() queued before run() is flushed first; an export on the current stream right after sees the final state"""
    from pixie_amd.mpm_solver import SceneBatch
    scs = [mpm_ball_scene(50_000, seed=30 + i, n_grid=40, scenario=("tree", "ball")[i]) for i in range(2)]
    batch, alone = zip(*[pair(sc) for sc in scs])
    sb = SceneBatch(batch)
    for k in range(3):
        batch[1].p2g2p(0, DT)
        alone[1].p2g2p(0, DT)
        sb.run(DT, 40)
        xs = [b.export_particle_x_to_torch().clone() for b in batch]    # no synchronisation in between
        for a in alone:
            a.run(DT, 40)
        for b, a, x in zip(batch, alone, xs):
            assert torch.equal(x, a.export_particle_x_to_torch())
            assert torch.equal(b.get_field("F_trial"), a.get_field("F_trial"))
            assert b.time == a.time
    sb.close()
    sb.close()


def test_full_size_eight_scenes(hip_device):
    """8 x 100 k particles in 50^3, 200 substeps: the batch that fills the chip"""
    from pixie_amd.mpm_solver import SceneBatch
    scs = [mpm_ball_scene(100_000, seed=40 + i, n_grid=50, scenario=("tree", "ball")[i % 2]) for i in range(8)]
    batch = [make(sc) for sc in scs]
    with SceneBatch(batch) as sb:
        sb.run(DT, 200)
    for i, (b, sc) in enumerate(zip(batch, scs)):
        a = make(sc)
        a.run(DT, 200)
        assert_same(b, a, f"scene {i}")
        assert np.isfinite(b.get_field("x").cpu().numpy()).all() and np.isfinite(b.get_field("v").cpu().numpy()).all()
        del a


def test_refusals_leave_every_scene_untouched(hip_device):
    from pixie_amd.mpm_solver import SceneBatch
    sc = mpm_ball_scene(10_000, seed=50, n_grid=32, scenario="ball")
    a, b, c = make(sc), make(sc), make(sc)
    a.run(DT, 5)
    x0 = [s.get_field("x").clone() for s in (a, b, c)]
    t0 = [s.time for s in (a, b, c)]

    def untouched():
        for s, x, t in zip((a, b, c), x0, t0):
            assert torch.equal(s.get_field("x"), x) and s.time == t

    with pytest.raises(ValueError):
        SceneBatch([a, b, a])
    with pytest.raises(ValueError):
        SceneBatch([])
    untouched()
    for _ in range(17):
        c.add_bounding_box()
    with pytest.raises(_lib.PixieHipError, match="boundary conditions"):
        SceneBatch([a, c])
    untouched()
    sb = SceneBatch([a, b])
    for _ in range(9):
        b.add_impulse_on_particles(force=[0.0, 0.0, 0.01], dt=DT, start_time=1.0)
    with pytest.raises(_lib.PixieHipError, match="particle modifiers"):
        sb.run(DT, 10)                # b changed after the batch was built: refused at the call, before anything ran
    untouched()
    with pytest.raises(_lib.PixieHipError, match="particle modifiers"):
        SceneBatch([b])
    sb.close()
    d, e = make(sc), make(sc)
    xd = d.get_field("x").clone()
    sb = SceneBatch([d, e])
    e.initialize(10_000, n_grid=32, grid_lim=2.0)         # a new handle: the batch no longer holds this scene
    with pytest.raises(_lib.PixieHipError, match="re-initialised"):
        sb.run(DT, 10)
    assert torch.equal(d.get_field("x"), xd) and d.time == 0.0
    sb.close()
    untouched()


def test_particles_leaving_the_grid_inside_a_batch(hip_device):
    """the scene of test_mpm_hip.py::test_particles_leaving_the_grid_freeze_with_a_defined_state as one member of a batch"""
    from pixie_amd.mpm_solver import SceneBatch
    sc = mpm_ball_scene(20000, seed=5, scenario="ball")
    sc["bcs"] = []
    sc["params"] = dict(sc["params"], g=[0.0, 0.0, 0.0])
    fast = np.arange(20000) % 50 == 0
    rng = np.random.default_rng(3)
    sc["x"] = sc["x"].copy()
    sc["x"][fast] = np.stack([np.full(400, 1.75), rng.uniform(0.6, 1.4, 400), rng.uniform(0.6, 1.4, 400)], 1).astype(np.float32)
    v0 = np.zeros((20000, 3), np.float32)
    v0[fast] = [25.0, 0.0, 0.0]

    def setup(s):
        s.set_field("v", v0)
        s._set_scalar("resort_interval", 4)

    other = mpm_ball_scene(30_000, seed=6, n_grid=40, scenario="tree")
    (lb, la), (ob, oa) = pair(sc, setup), pair(other)
    with SceneBatch([ob, lb]) as sb:
        sb.run(sc["dt"], 300)
        la.run(sc["dt"], 300)
        oa.run(sc["dt"], 300)
        assert_same(lb, la, "leaving")
        assert_same(ob, oa, "other")
        assert int((lb.get_field("selection").cpu().numpy() == 2).sum()) == 400
        sb.run(sc["dt"], 50)
        la.run(sc["dt"], 50); oa.run(sc["dt"], 50)
        assert_same(lb, la, "leaving, after")
        assert_same(ob, oa, "other, after")


def test_the_batched_kernels_are_the_launches(hip_device):
    """The bit comparisons above would also pass for a batch step that looped pixie_mpm_step per scene: the kernel trace of a batched
    call must show the batched block / grid kernels and no solo block / grid kernel."""
    from torch.profiler import ProfilerActivity, profile
    from pixie_amd.mpm_solver import SceneBatch
    scs = [mpm_ball_scene(20_000, seed=60 + i, n_grid=40, scenario="ball") for i in range(3)]
    batch = [make(sc) for sc in scs]
    with SceneBatch(batch) as sb:
        sb.run(DT, 5)                  # first binning outside the trace
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            sb.run(DT, 10)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "mpm_" in e.name]
    batched = [n for n in names if "batch_kernel" in n]
    solo = [n for n in names if "mpm_block_kernel<" in n or "mpm_grid_block_kernel<" in n]
    print(f"{len(batched)} batched launches, {len(solo)} solo launches")
    assert sum("mpm_grid_block_batch_kernel" in n for n in batched) == 10      # one grid launch per substep for the three scenes
    nb = sum("mpm_block_batch_kernel" in n for n in batched)
    assert nb == 11 * len({(int(x._get_scalar("item_cap")), int(x._get_scalar("scatter_bits"))) for x in batch})   # P2G, 9 fused, G2P per group
    assert not solo
