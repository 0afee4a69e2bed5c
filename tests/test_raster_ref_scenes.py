"""The scenes of the rasteriser tests (tests/_raster_ref.py: scene()) are fit to compare on: in the helper's float64 run at most
0.5 % of the pixels and 0.5 % of the Gaussians are borderline.  A condition on the inputs (seeds and sizes), not a measurement of
the code under test.  The larger scenes (b, c) are checked the same way where they run, in tests/test_raster_hip.py."""
import numpy as np
import pytest

from tests import _raster_ref as rr


@pytest.mark.parametrize("name", rr.CPU_SCENES)
def test_borderline_share(name):
    s = rr.scene(name)
    cam = s["cam"]
    assert cam["W"] <= 128 and cam["H"] <= 128 and len(s["means"]) <= 5000
    r64, r32, y = rr.yardstick(s)
    bp, bg = r64["borderline_pixels"], r64["borderline_gaussians"]
    n = max(len(bg), 1)
    print(f"scene {name}: {len(bg)} Gaussians ({int((r64['radii'] > 0).sum())} visible), {cam['W']}x{cam['H']}, borderline pixels "
          f"{int(bp.sum())}/{bp.size}, Gaussians {int(bg.sum())}/{len(bg)}, float32 yardstick y = {y:.3e}, "
          f"max n_contrib {int(r64['n_contrib'].max())}")
    assert bp.sum() <= 0.005 * bp.size and bg.sum() <= 0.005 * n
    assert y <= rr.Y_CAP, "a float32 / float64 decision flip escaped the borderline sets"
    assert np.isfinite(r64["color"]).all() and np.isfinite(r32["color"]).all()
    # the scene shows what it is meant to show
    vis = int((r64["radii"] > 0).sum())
    if name in ("f", "h"):
        assert vis == 0 and np.array_equal(r64["color"], np.broadcast_to(s["bg"].astype(np.float64)[:, None, None], r64["color"].shape))
    if name == "g":
        assert 0.1 * len(bg) < vis < 0.9 * len(bg)
    if name == "e":
        assert (r64["n_contrib"] == 1).all()
    if name == "d":
        assert (r64["final_T"] < 0.011).mean() > 0.2               # many pixels ran into the termination rule
    if name == "i":
        assert r64["n_contrib"].max() > 2 * 256
    if name == "a":
        assert vis > 0.5 * len(bg) and y > 0
