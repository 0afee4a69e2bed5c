"""GPU tests of per-scene time steps and frame schedules in the fused multi-scene step (SceneBatch.run with per-scene sequences,
SceneBatch.run_frames, C ABI pixie_mpm_batch_run): every scene must end -- state and exported frames -- in exactly the bits of its
solo loop, the scenes must share the launches of each global step, and refusals must leave every scene untouched."""
import math

import numpy as np
import pytest
import torch

from pixie_amd import _lib
from pixie_amd.synthetic import mpm_ball_scene
from tests.test_mpm_batch_hip import DT, assert_same, heterogeneous_scenes, make

pytestmark = pytest.mark.gpu

WINDOW = 1024       # kBatchWindow of csrc/mpm.hip: global steps per uploaded table window


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return torch.from_numpy(q.astype(np.float32))


def solo_frames(s, q):
    """the reference frame loop (gs_simulation.py:573-634): export, then steps_per_frame substeps"""
    pos, cov = [], []
    for _ in range(q.n_frames):
        p, c = s.export_frame_for_rendering(q.gs_num, q.scale_origin, q.original_mean_pos, q.rotation_matrices, q.z_shift_value,
                                            q.with_cov)
        pos.append(p.clone())
        cov.append(c.clone() if c is not None else None)
        s.run(q.dt, q.steps_per_frame)
    return pos, cov


def assert_frames(got, pos, cov, q, tag):
    gp, gc = got
    assert tuple(gp.shape) == (q.n_frames, q.gs_num, 3), tag
    assert (gc is None) == (not q.with_cov), tag
    for f in range(q.n_frames):
        assert torch.equal(gp[f], pos[f]), f"{tag}: pos of frame {f}"
        if q.with_cov:
            assert torch.equal(gc[f], cov[f]), f"{tag}: cov of frame {f}"


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "mpm_" in e.name or "frame_export" in e.name]


def count(names, key):
    return sum(key in n for n in names)


def test_per_scene_dt_and_counts_equal_solo_runs(hip_device):
    from pixie_amd.mpm_solver import SceneBatch
    scs = heterogeneous_scenes()
    batch = [make(sc) for sc in scs]
    alone = [make(sc) for sc in scs]
    calls = [((1e-4, 2e-5, 1e-5, 1e-4), (40, 200, 400, 0)),
             ((2e-5, 1e-4, 1e-4, 1e-5), (150, 30, 0, 120))]
    with SceneBatch(batch) as sb:
        for call, (dts, ns) in enumerate(calls):
            before = [(b.time, b.get_field("x").clone()) for b in batch]
            sb.run(list(dts), list(ns))
            for a, d, n in zip(alone, dts, ns):
                a.run(d, n)
            for i, (b, a) in enumerate(zip(batch, alone)):
                assert_same(b, a, f"call {call} scene {i}")
                if ns[i] == 0:
                    assert b.time == before[i][0] and torch.equal(b.get_field("x"), before[i][1]), f"call {call} scene {i} moved"
    assert [b.time > 0.0 for b in batch] == [True] * 4
    for b in batch:
        assert np.isfinite(b.get_field("x").cpu().numpy()).all()


def frame_scenes():
    from pixie_amd.mpm_solver import FrameSchedule
    tree = mpm_ball_scene(20_000, seed=70, n_grid=40, scenario="tree")
    ball = mpm_ball_scene(30_000, seed=71, n_grid=48, scenario="ball")
    snow = heterogeneous_scenes()[3]                       # moving cuboid
    Rs = [rotation(1), rotation(2)]
    scheds = [FrameSchedule(1e-4, 7, 5, gs_num=20_000, scale_origin=0.37, original_mean_pos=torch.tensor([0.1, -0.2, 0.3]),
                            rotation_matrices=Rs, z_shift_value=0.1, with_cov=True),
              FrameSchedule(5e-5, 13, 3, gs_num=10_000, scale_origin=1.7, original_mean_pos=[0.5, 0.5, 0.0],
                            rotation_matrices=Rs[:1], z_shift_value=0.0, with_cov=False),
              FrameSchedule(1e-5, 20, 4, gs_num=20_000, scale_origin=0.8, original_mean_pos=[0.0, 0.0, 0.0],
                            rotation_matrices=[], z_shift_value=-0.05, with_cov=True)]
    return [tree, ball, snow], scheds


def test_frames_equal_the_reference_frame_loop(hip_device):
    from pixie_amd.mpm_solver import SceneBatch
    scs, scheds = frame_scenes()
    batch = [make(sc) for sc in scs]
    alone = [make(sc) for sc in scs]
    with SceneBatch(batch) as sb:
        for call in range(2):
            got = sb.run_frames(scheds)
            for i, (a, q) in enumerate(zip(alone, scheds)):
                pos, cov = solo_frames(a, q)
                assert_frames(got[i], pos, cov, q, f"call {call} scene {i}")
                assert_same(batch[i], a, f"call {call} scene {i}")
        # preallocated outputs
        out = [(torch.full((q.n_frames, q.gs_num, 3), float("nan"), device=hip_device),
                torch.full((q.n_frames, q.gs_num, 6), float("nan"), device=hip_device) if q.with_cov else None) for q in scheds]
        got = sb.run_frames(scheds, out=out)
        for i, (a, q) in enumerate(zip(alone, scheds)):
            assert got[i][0] is out[i][0] and got[i][1] is out[i][1]
            pos, cov = solo_frames(a, q)
            assert_frames(got[i], pos, cov, q, f"out= scene {i}")
            assert_same(batch[i], a, f"out= scene {i}")


def launch_check(names, scheds):
    """grid launches = max total substeps; batched export launches = distinct global steps that carry an export; no solo kernel"""
    totals = [q.steps_per_frame * q.n_frames for q in scheds]
    steps = set()
    for q in scheds:
        if q.gs_num > 0 and q.n_frames > 0:
            steps.update(f * q.steps_per_frame for f in range(q.n_frames))
    assert count(names, "mpm_grid_block_batch_kernel") == max(totals)
    assert count(names, "frame_export_batch_kernel") == len(steps)
    assert not [n for n in names if "mpm_block_kernel<" in n or "mpm_grid_block_kernel<" in n or "frame_export_kernel" in n]


def test_schedule_shares_launches(hip_device):
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    scs = [mpm_ball_scene(20_000, seed=80 + i, n_grid=40, scenario=("tree", "ball", "ball")[i]) for i in range(3)]
    batch = [make(sc) for sc in scs]
    scheds = [FrameSchedule(1e-4, 5, 3, gs_num=20_000), FrameSchedule(2e-5, 7, 2, gs_num=5_000, with_cov=False),
              FrameSchedule(5e-5, 4, 4, gs_num=20_000)]
    with SceneBatch(batch) as sb:
        sb.run(DT, 5)                  # first binning outside the trace
        names = kernel_names(lambda: sb.run_frames(scheds))
        print(f"{count(names, 'mpm_grid_block_batch_kernel')} grid launches, {count(names, 'frame_export_batch_kernel')} export launches, "
              f"{count(names, 'mpm_block_batch_kernel')} block launches")
        launch_check(names, scheds)
        # a ragged run: one grid launch per global step, scenes drop out
        names = kernel_names(lambda: sb.run([1e-4, 2e-5, 5e-5], [12, 30, 0]))
        assert count(names, "mpm_grid_block_batch_kernel") == 30
        assert not [n for n in names if "mpm_block_kernel<" in n or "mpm_grid_block_kernel<" in n]


def test_long_schedule_crosses_table_windows(hip_device):
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    scs = []
    for i in range(2):
        sc = mpm_ball_scene(4_000, seed=90 + i, n_grid=24, scenario="ball")
        sc["bcs"] = [dict(type="bounding_box"),
                     dict(type="cuboid", point=[1.0, 1.0, 0.55], size=[0.3, 0.3, 0.05], velocity=[0.0, 0.2, 0.1], start_time=0.0,
                          end_time=0.03, reset=1)]
        scs.append(sc)
    batch = [make(sc) for sc in scs]
    alone = [make(sc) for sc in scs]
    scheds = [FrameSchedule(1e-5, 700, 3, gs_num=4_000), FrameSchedule(2e-5, 1150, 2, gs_num=4_000, with_cov=False)]
    assert max(q.steps_per_frame * q.n_frames for q in scheds) > 2 * WINDOW
    with SceneBatch(batch) as sb:
        got = sb.run_frames(scheds)
        sb.run([1e-5, 2e-5], [2 * WINDOW + 5, WINDOW - 1])
    for i, (a, q) in enumerate(zip(alone, scheds)):
        pos, cov = solo_frames(a, q)
        assert_frames(got[i], pos, cov, q, f"scene {i}")
    alone[0].run(1e-5, 2 * WINDOW + 5)
    alone[1].run(2e-5, WINDOW - 1)
    for i, (b, a) in enumerate(zip(batch, alone)):
        assert_same(b, a, f"scene {i}")


def test_equal_dt_frames_match_scalar_run(hip_device):
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    scs = [mpm_ball_scene(20_000, seed=100 + i, n_grid=40, scenario=("tree", "ball")[i % 2]) for i in range(3)]
    framed = [make(sc) for sc in scs]
    scalar = [make(sc) for sc in scs]
    scheds = [FrameSchedule(DT, 10, 3, gs_num=20_000) for _ in scs]
    with SceneBatch(framed) as fb, SceneBatch(scalar) as sb:
        fb.run(DT, 5)
        sb.run(DT, 5)

        def per_frame():
            for _ in range(3):
                sb.run(DT, 10)

        names_f = kernel_names(lambda: fb.run_frames(scheds))
        names_s = kernel_names(per_frame)
    for i, (f, s) in enumerate(zip(framed, scalar)):
        assert_same(f, s, f"scene {i}")
    launch_check(names_f, scheds)
    assert count(names_f, "mpm_grid_block_batch_kernel") == count(names_s, "mpm_grid_block_batch_kernel") == 30
    assert count(names_f, "mpm_block_batch_kernel") == count(names_s, "mpm_block_batch_kernel")
    assert count(names_s, "frame_export_batch_kernel") == 0 and count(names_f, "frame_export_batch_kernel") == 3


def test_schedule_refusals_leave_scenes_untouched(hip_device):
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    sc = mpm_ball_scene(10_000, seed=110, n_grid=32, scenario="ball")
    a, b = make(sc), make(sc)
    a.run(DT, 5)
    x0 = [s.get_field("x").clone() for s in (a, b)]
    t0 = [s.time for s in (a, b)]
    r0 = [int(s._get_scalar("n_rebins")) for s in (a, b)]

    def untouched():
        for s, x, t, r in zip((a, b), x0, t0, r0):
            assert torch.equal(s.get_field("x"), x) and s.time == t and int(s._get_scalar("n_rebins")) == r

    sb = SceneBatch([a, b])
    for dt in (0.0, -DT, math.inf, math.nan):
        with pytest.raises(_lib.PixieHipError, match="dt"):
            sb.run([DT, dt], 10)
        untouched()
        with pytest.raises(_lib.PixieHipError, match="dt"):
            sb.run_frames([FrameSchedule(DT, 5, 2), FrameSchedule(dt, 5, 2, gs_num=100)])
        untouched()
    with pytest.raises(_lib.PixieHipError, match="negative"):
        sb.run(DT, [10, -1])
    for spf, nf in ((-1, 2), (5, -2)):
        with pytest.raises(_lib.PixieHipError, match="negative"):
            sb.run_frames([FrameSchedule(DT, 5, 2), FrameSchedule(DT, spf, nf)])
    untouched()
    with pytest.raises(ValueError):
        sb.run([DT, DT, DT], 10)
    with pytest.raises(ValueError):
        sb.run(DT, [10])
    with pytest.raises(ValueError):
        sb.run_frames([FrameSchedule(DT, 5, 2)])
    with pytest.raises(ValueError):
        sb.run_frames([FrameSchedule(DT, 5, 2, gs_num=10), FrameSchedule(DT, 5, 2)], out=[(torch.empty(2, 10, 3, device=hip_device), None)])
    with pytest.raises(_lib.PixieHipError, match="n_out"):
        sb.run_frames([FrameSchedule(DT, 5, 2), FrameSchedule(DT, 5, 2, gs_num=10_001)])
    untouched()
    # the C entry point's own checks: a wrong schedule count, a null d_pos with n_out > 0
    arr = (_lib.BatchSched * 2)()
    for q in arr:
        q.dt, q.steps_per_chunk, q.n_chunks, q.scale = DT, 5, 2, 1.0
    arr[1].n_out = 10
    with torch.cuda.device(hip_device):
        assert sb._L.pixie_mpm_batch_run(sb._b, arr, 2, _lib.current_stream_ptr()) != 0
        assert b"null d_pos" in sb._L.pixie_last_error()
        arr[1].n_out = 0
        assert sb._L.pixie_mpm_batch_run(sb._b, arr, 3, _lib.current_stream_ptr()) != 0
        assert b"schedules" in sb._L.pixie_last_error()
    untouched()
    # what batch_check_handle refuses, through both calls
    for _ in range(9):
        b.add_impulse_on_particles(force=[0.0, 0.0, 0.01], dt=DT, start_time=1.0)
    with pytest.raises(_lib.PixieHipError, match="particle modifiers"):
        sb.run([DT, DT], [10, 0])
    with pytest.raises(_lib.PixieHipError, match="particle modifiers"):
        sb.run_frames([FrameSchedule(DT, 5, 2, gs_num=100), FrameSchedule(DT, 0, 0)])
    untouched()
    sb.close()
