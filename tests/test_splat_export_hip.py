"""GPU tests of the per-frame 3DGS splat export (gs_simulation.py:253-322): the device decomposition pixie_splat_from_cov against the
reference's cov3D_to_log_scales_and_quats (tests/golden/splat_export.npz), the fused single-scene export (export_frame_splats), the
batched one (SceneBatch.run_frames with FrameSchedule.with_splats), the PLY writer end to end, and the refusals of the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pixie_amd import _lib, ply_io
from tests import _splat_checks as sc
from tests.test_mpm_batch_hip import assert_same, heterogeneous_scenes, make
from tests.test_mpm_batch_schedule_hip import rotation

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def eigh64(c6):
    w, v = np.linalg.eigh(sc.sym(c6))
    return w[:, ::-1].copy(), v[:, :, ::-1].copy()


def jelly_state():
    """scene jelly_apic of mpm_ref_golden.npz in its state after 6 substeps (as test_mpm_hip.test_export_frame_for_rendering)"""
    from tests._mpm_ref_driver import load_fixture
    from pixie_amd.mpm_solver import MPM_Simulator_WARP
    g = np.load(os.path.join(HERE, "frame_export.npz"))
    scene, arrays, ref = load_fixture(os.path.join(HERE, "mpm_ref_golden.npz"))["jelly_apic"]
    h = MPM_Simulator_WARP(10)
    h.load_initial_data_from_torch(torch.from_numpy(arrays["x0"]), torch.from_numpy(arrays["vol"]), torch.from_numpy(arrays["cov"]),
                                   n_grid=scene["n_grid"], grid_lim=scene["grid_lim"])
    h.set_field("x", ref["k6/x"].astype(np.float32))
    h.set_field("F_trial", ref["k6/F_trial"].astype(np.float32).reshape(-1, 9))
    args = (int(g["gs_num"]), float(g["scale_origin"]), torch.tensor(g["mean"]), [torch.tensor(R) for R in g["rot_f64"]])
    return h, args, float(g["z_shift"])


def test_cov3D_to_log_scales_and_quats_meets_the_bars(hip_device):
    from pixie_amd.splat_export import cov3D_to_log_scales_and_quats
    g = sc.golden()
    for tag in ("frame", "synth"):
        c6 = g[f"{tag}/cov"]
        ls, q = cov3D_to_log_scales_and_quats(torch.from_numpy(c6).to(hip_device))
        assert ls.device == q.device == hip_device and ls.dtype == q.dtype == torch.float32
        checked, e_lam, e_rec = sc.check_splats(c6, ls.cpu().numpy(), q.cpu().numpy(), g[f"{tag}/eigh64_w"], g[f"{tag}/eigh64_v"],
                                                g[f"{tag}/ref_f32_log_scale"], g[f"{tag}/ref_f32_quat"], what=tag)
        print(f"device {tag}: eigenvalue err {e_lam:.2e}, reconstruction err {e_rec:.2e}, {checked} eigenvectors compared")
    ls, q = cov3D_to_log_scales_and_quats(torch.empty((0, 6), device=hip_device))
    assert ls.shape == (0, 3) and q.shape == (0, 4)


def test_export_frame_splats_single_launch_bits(hip_device):
    from pixie_amd.splat_export import cov3D_to_log_scales_and_quats
    h, args, z = jelly_state()
    pos0, cov0 = h.export_frame_for_rendering(*args, z_shift_value=z)
    pos, cov, ls, q = h.export_frame_splats(*args, z_shift_value=z)
    assert torch.equal(pos, pos0) and torch.equal(cov, cov0)
    ls1, q1 = cov3D_to_log_scales_and_quats(cov)
    assert torch.equal(ls, ls1) and torch.equal(q, q1)
    c6 = cov.cpu().numpy()
    w, v = eigh64(c6)
    sc.check_splats(c6, ls.cpu().numpy(), q.cpu().numpy(), w, v, what="jelly_apic frame")


def splat_schedules():
    from pixie_amd.mpm_solver import FrameSchedule
    scs = heterogeneous_scenes()
    jelly, sand, snow = scs[0], scs[2], scs[3]
    Rs = [rotation(5), rotation(6)]
    scheds = [FrameSchedule(1e-4, 6, 4, gs_num=5_000, scale_origin=0.37, original_mean_pos=[0.1, -0.2, 0.3], rotation_matrices=Rs,
                            z_shift_value=0.1, with_cov=False, with_splats=True),
              FrameSchedule(5e-5, 9, 3, gs_num=60_000, scale_origin=1.3, original_mean_pos=[0.0, 0.5, 0.0], rotation_matrices=Rs[:1]),
              FrameSchedule(1e-5, 10, 3, gs_num=20_000, scale_origin=0.8, z_shift_value=-0.05, with_splats=True)]
    return [jelly, sand, snow], scheds


def solo_splat_frames(s, q):
    out = []
    for _ in range(q.n_frames):
        if q.with_splats:
            out.append(tuple(t.clone() for t in s.export_frame_splats(q.gs_num, q.scale_origin, q.original_mean_pos, q.rotation_matrices,
                                                                      q.z_shift_value)))
        else:
            p, c = s.export_frame_for_rendering(q.gs_num, q.scale_origin, q.original_mean_pos, q.rotation_matrices, q.z_shift_value,
                                                q.with_cov)
            out.append((p.clone(), c.clone() if c is not None else None))
        s.run(q.dt, q.steps_per_frame)
    return out


def export_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "mpm_" in e.name or "frame_" in e.name]


def n_of(names, key):
    return sum(key in n for n in names)


def test_batched_splat_frames(hip_device):
    import dataclasses
    from pixie_amd.mpm_solver import SceneBatch
    scs, scheds = splat_schedules()
    batch = [make(s) for s in scs]
    alone = [make(s) for s in scs]
    plain = [make(s) for s in scs]
    plain_scheds = [dataclasses.replace(q, with_splats=False, with_cov=True) for q in scheds]
    with SceneBatch(batch) as sb, SceneBatch(plain) as pb:
        names = export_names(lambda: sb.run_frames(scheds))
        got = sb.run_frames(scheds)                               # a second call: the frames after the first's
        got_plain = [pb.run_frames(plain_scheds) for _ in range(2)][1]
    for i, (a, q) in enumerate(zip(alone, scheds)):
        solo_splat_frames(a, q)                                   # the profiled call
        ref = solo_splat_frames(a, q)
        assert len(got[i]) == (4 if q.with_splats else 2)
        for k, t in enumerate(got[i]):
            if t is None:
                continue
            assert tuple(t.shape) == (q.n_frames, q.gs_num, (3, 6, 3, 4)[k]), (i, k)
            for f in range(q.n_frames):
                assert torch.equal(t[f], ref[f][k]), f"scene {i} output {k} frame {f}"
        assert torch.equal(got[i][0], got_plain[i][0]), f"scene {i}: pos differs from the with_splats=False run"
        if got[i][1] is not None:
            assert torch.equal(got[i][1], got_plain[i][1]), f"scene {i}: cov differs from the with_splats=False run"
        assert_same(batch[i], a, f"scene {i}")
        assert_same(plain[i], a, f"scene {i} (plain)")
    # launches: no solo export; per export step one launch for the scenes without splats and one for those with
    assert not [n for n in names if "frame_export_kernel" in n or "frame_splat_kernel" in n]
    plain_steps, splat_steps = set(), set()
    for q in scheds:
        (splat_steps if q.with_splats else plain_steps).update(f * q.steps_per_frame for f in range(q.n_frames))
    assert n_of(names, "frame_export_batch_kernel") == len(plain_steps)
    assert n_of(names, "frame_splat_batch_kernel") == len(splat_steps)
    assert n_of(names, "frame_export_batch_kernel") + n_of(names, "frame_splat_batch_kernel") <= 2 * len(plain_steps | splat_steps)
    print(f"{len(plain_steps | splat_steps)} export steps: {n_of(names, 'frame_export_batch_kernel')} export + "
          f"{n_of(names, 'frame_splat_batch_kernel')} splat launches")


def test_no_splat_scene_keeps_todays_launches(hip_device):
    """run_frames without splats, and pixie_mpm_batch_run_splats with every splat entry empty, issue the same launches in the same order"""
    from pixie_amd.mpm_solver import SceneBatch
    scs, scheds = splat_schedules()
    import dataclasses
    scheds = [dataclasses.replace(q, with_splats=False) for q in scheds]
    a, b = [make(s) for s in scs], [make(s) for s in scs]
    with SceneBatch(a) as sa, SceneBatch(b) as sb:
        names_a = export_names(lambda: sa.run_frames(scheds))
        orig = sb._call

        def via_splats(name, arr, n):
            assert name == "pixie_mpm_batch_run"
            return orig("pixie_mpm_batch_run_splats", arr, (_lib.BatchSplatOut * n)(), n)
        sb._call = via_splats
        names_b = export_names(lambda: sb.run_frames(scheds))
    assert names_a == names_b and n_of(names_a, "frame_splat") == 0 and n_of(names_a, "frame_export_batch_kernel") > 0
    for x, y in zip(a, b):
        assert_same(x, y)


@pytest.mark.parametrize("to_original_coord", [True, False])
def test_export_gaussians_to_ply_end_to_end(hip_device, tmp_path, to_original_coord):
    from pixie_amd.splat_export import export_gaussians_to_ply
    h, (gs_num, scale, mean, rots), z = jelly_state()
    g = torch.Generator().manual_seed(3)
    opacity = torch.sigmoid(torch.randn((gs_num + 7, 1), generator=g)).to(hip_device)          # activated, as the driver passes it
    shs = torch.randn((gs_num + 7, 16, 3), generator=g).to(hip_device)
    path = export_gaussians_to_ply(str(tmp_path / "ply_files"), h, 3, gs_num, scale, rots, opacity, shs, 3, {"z_shift_value": z}, mean,
                                   to_original_coord=to_original_coord)
    assert path == str(tmp_path / "ply_files" / "frame_00003.ply")
    v, _ = ply_io.read_ply(path)
    names = [str(n) for n in sc.golden()["ply3/names"]]
    assert list(v.dtype.names) == names and len(v) == gs_num and all(v.dtype[n] == np.dtype("f4") for n in names)
    col = lambda pre, n: np.stack([v[f"{pre}{i}"] for i in range(n)], 1)
    pos_r, cov = h.export_frame_for_rendering(gs_num, scale, mean, rots, z_shift_value=z)
    pos = pos_r if to_original_coord else h.export_particle_x_to_torch()[:gs_num]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pos.cpu().numpy())
    assert not np.stack([v["nx"], v["ny"], v["nz"]], 1).any()
    sh = shs[:gs_num].cpu()
    assert np.array_equal(col("f_dc_", 3), sh[:, :1, :].transpose(1, 2).flatten(1).numpy())
    assert np.array_equal(col("f_rest_", 45), sh[:, 1:, :].transpose(1, 2).flatten(1).numpy())
    assert np.array_equal(v["opacity"], opacity[:gs_num, 0].cpu().numpy())
    c6 = cov.cpu().numpy()
    w, vec = eigh64(c6)
    sc.check_splats(c6, col("scale_", 3), col("rot_", 4), w, vec, what=f"ply to_original_coord={to_original_coord}")


def test_refusals(hip_device):
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    from pixie_amd.splat_export import cov3D_to_log_scales_and_quats
    L = _lib.load()
    st = _lib.current_stream_ptr()
    t = torch.zeros((8, 6), device=hip_device)
    p = lambda x: C.c_void_p(x.data_ptr())
    assert L.pixie_splat_from_cov(p(t), -1, p(t), p(t), st) != 0 and b"< 0" in L.pixie_last_error()
    assert L.pixie_splat_from_cov(p(t), 8, None, p(t), st) != 0 and b"null pointer" in L.pixie_last_error()
    with pytest.raises(ValueError, match="HIP device"):
        cov3D_to_log_scales_and_quats(t.cpu())
    with pytest.raises(ValueError, match="float32"):
        cov3D_to_log_scales_and_quats(t.double())

    h, (gs_num, scale, mean, rots), z = jelly_state()
    out = [torch.empty((gs_num, k), device=hip_device) for k in (3, 6, 3, 4)]
    d3 = lambda v: (C.c_double * 3)(*v)
    M = (C.c_double * 9)(*np.eye(3).reshape(-1))
    for k in range(4):
        ptrs = [p(o) if j != k else None for j, o in enumerate(out)]
        assert L.pixie_mpm_export_frame_splats(h._h, gs_num, d3([1, 1, 1]), 1.0, d3([0, 0, 0]), M, *ptrs, st) != 0
        assert b"null output" in L.pixie_last_error()
    with pytest.raises(_lib.PixieHipError, match="bad n_out"):
        h.export_frame_splats(0, scale, mean, rots)

    s = make(heterogeneous_scenes()[0])
    s.run(1e-4, 3)
    x0, t0 = s.get_field("x").clone(), s.time
    with SceneBatch([s]) as sb:
        arr = (_lib.BatchSched * 1)()
        arr[0].dt, arr[0].steps_per_chunk, arr[0].n_chunks, arr[0].scale = 1e-4, 5, 2, 1.0
        pos = torch.empty((2, 100, 3), device=hip_device)
        cov = torch.empty((2, 100, 6), device=hip_device)
        ls = torch.empty((2, 100, 3), device=hip_device)
        q = torch.empty((2, 100, 4), device=hip_device)
        spl = (_lib.BatchSplatOut * 1)()
        cases = [((100, pos, cov), (ls, None), b"only one of"), ((100, pos, cov), (None, q), b"only one of"),
                 ((0, None, None), (ls, q), b"n_out 0"), ((100, pos, None), (ls, q), b"need d_cov")]
        with torch.cuda.device(hip_device):
            for (n_out, dp, dc), (dl, dq), msg in cases:
                arr[0].n_out = n_out
                arr[0].d_pos = dp.data_ptr() if dp is not None else None
                arr[0].d_cov = dc.data_ptr() if dc is not None else None
                spl[0].d_log_scale = dl.data_ptr() if dl is not None else None
                spl[0].d_quat = dq.data_ptr() if dq is not None else None
                assert L.pixie_mpm_batch_run_splats(sb._b, arr, spl, 1, _lib.current_stream_ptr()) != 0, msg
                assert msg in L.pixie_last_error(), (msg, L.pixie_last_error())
        with pytest.raises(ValueError, match="4-tuple"):
            sb.run_frames([FrameSchedule(1e-4, 5, 2, gs_num=100, with_splats=True)], out=[(pos, cov)])
        assert torch.equal(s.get_field("x"), x0) and s.time == t0
