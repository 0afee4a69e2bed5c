"""CPU checks of the backward-pass oracle itself (tests/_raster_grad_ref.py): its float64 forward is the NumPy helper's, and its
float64 gradients are the derivatives of its own float64 loss by central finite differences."""
import numpy as np
import pytest

from tests import _raster_ref as rr
from tests import _raster_grad_ref as gr


@pytest.mark.parametrize("name", ("e", "g", "w"))
def test_float64_forward_equals_the_numpy_helper(name):
    s, kw, w, share = gr.case(name)
    r64 = rr.render(s, np.float64, cov6=kw["cov6"])
    got = gr.run(s, np.float64, w, grad=False, **kw)
    keep = ~r64["borderline_pixels"]
    assert share <= gr.MAX_ZERO_SHARE
    assert np.max(np.abs(got["color"] - r64["color"])[:, keep], initial=0.0) <= 1e-14
    assert got["n_contrib_max"] == int(r64["n_contrib"][keep].max(initial=0))


@pytest.mark.parametrize("form,degree", (("cov", None), ("sr", 3)))
def test_float64_gradients_against_central_differences(form, degree):
    """>= 20 coordinates of every input on a scene of <= 200 Gaussians at 48 x 48.  The step 1e-6 changes the loss by ~1e-6 |g| against
    a float64 rounding floor of ~1e-15, and its truncation error is ~1e-12 times the third derivative; no decision of the render may
    differ between the base run and the two perturbed runs, which the signature (every mask of the render) asserts."""
    s, kw, w, share = gr.case("small", form, degree)
    assert len(s["means"]) <= 200 and s["cam"]["W"] == 48 and s["cam"]["H"] == 48 and share <= gr.MAX_ZERO_SHARE
    base = gr.run(s, np.float64, w, **kw)
    rng = np.random.default_rng(5)
    live = np.nonzero(np.abs(base["grads"]["opacities"]) > 0)[0]
    assert len(live) >= 20
    h = 1.0e-6
    for q, g in base["grads"].items():
        shape = (len(s["means"]), 2) if q == "means2D" else g.shape
        scale = (0.5 * s["cam"]["W"], 0.5 * s["cam"]["H"]) if q == "means2D" else None
        top = float(np.abs(g).max())
        assert top > 0, q
        checked = 0
        for i in rng.choice(live, size=20, replace=False):
            sub = tuple(int(rng.integers(0, d)) for d in shape[1:])
            off = np.zeros(shape)
            off[(int(i),) + sub] = h
            plus = gr.run(s, np.float64, w, grad=False, offsets={q: off}, **kw)
            minus = gr.run(s, np.float64, w, grad=False, offsets={q: -off}, **kw)
            assert plus["signature"] == base["signature"] == minus["signature"], f"{q}[{i}]: the step flips a decision"
            fd = (plus["loss"] - minus["loss"]) / (2 * h)
            want = g[(int(i),) + sub] / (scale[sub[0]] if scale else 1.0)
            assert abs(fd - want) <= 1e-6 * abs(want) + 1e-8 * top, (q, int(i), sub, fd, want)
            checked += 1
        assert checked >= 20
