"""bench.py's plain run: the headline step alone, its result line, and --dump-outputs (what the timed path returned in its
last step, for comparing two builds output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def run_bench(*extra, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *extra], capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_dry_run_is_the_headline_step_alone():
    rec = run_bench("--steps", "4", "--warmup", "1", "--dry-run", timeout=300)
    for k in CONTRACT:
        assert k in rec, k
    assert rec["steps"] == 4 and rec["ms_per_step"] > 0 and rec["higher_is_better"] is True
    for k in ("mpm", "mpm_1m", "exact_f32", "cpu_baseline", "pipeline_ms_per_scene", "field_to_particles_ms"):
        assert k not in rec, k


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_step_returned(hip_device, tmp_path):
    """A 16^3 grid fits whole (no sampling): the dumped arrays are the outputs of the same networks on the same seeded input,
    recomputed here."""
    from pixie_amd.synthetic import feature_grid
    from pixie_amd.unet import RegressionUNet, SegmentationUNet, predict_material_field
    from pixie_amd.unet_plan import synthetic_state_dict
    D = 16
    rec = run_bench("--steps", "2", "--warmup", "1", "--grid", str(D), "--dump-outputs", str(tmp_path))
    for k in CONTRACT:
        assert k in rec, k
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and "mpm" not in rec
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("combined", "seg_pred", "seg_logits", "cont_pred")}
    assert sum(os.path.getsize(tmp_path / f"{n}.npy") for n in got) < 64e6
    assert all(a.dtype == np.float32 for a in got.values())

    kw = dict(feature_channels=64, cond_dim=32, model_channels=64, num_res_blocks=3, channel_mult=(1, 1, 2, 4),
              attention_resolutions=(), grid_size=D)
    seg, cont = SegmentationUNet(num_classes=8, **kw), RegressionUNet(out_channels=3, **kw)
    seg.load_numpy_state(synthetic_state_dict(seg.cfg, 0)); cont.load_numpy_state(synthetic_state_dict(cont.cfg, 1000))
    seg, cont = seg.to(hip_device).eval(), cont.to(hip_device).eval()
    feat = torch.from_numpy(feature_grid(D, 64, seed=100)).to(hip_device)
    want = dict(zip(("combined", "seg_pred", "seg_logits", "cont_pred"), predict_material_field(seg, cont, feat)))
    for name, a in got.items():
        w = want[name].reshape(-1, D ** 3).float().cpu().numpy()
        assert a.shape == w.shape, (name, a.shape, w.shape)
        if name == "seg_pred":
            assert (a == w).mean() > 0.999
        else:
            assert np.linalg.norm(a - w) <= 1e-5 * np.linalg.norm(w), name
