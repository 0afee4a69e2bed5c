"""CPU checks of pixie_amd/csrc/raster_grad_math.h (compiled for the host by tests/host_harness/raster_grad_math_host.cpp, g++ -O2
-ffp-contract=off) against the float64 gradients of the torch oracle tests/_raster_grad_ref.py, on whole small scenes.

Bar, per quantity q (rel-L2 over all Gaussians): let y_q be the oracle's own float32-against-float64 distance; the header must lie
within 3 y_q + 2 K 2^-24 of the float64 gradient, K being the scene's largest n_contrib.  3 is the room every raster test here gives
a different but equally valid float32 rounding sequence; 2 K 2^-24 is the derived relative error of a K-step chain of T / (1 - alpha)
recoveries at two roundings a step.  The header walks front to back with the forward's T sequence and has no such chain, so it should
sit near y_q.  err / y_q is printed per scene and quantity (-s)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _raster_grad_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "raster_grad_math_host.cpp")
FP = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(FP) if a is not None else None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("raster_grad_host") / "libraster_grad_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_raster_grad.restype = C.c_int
    h.hh_raster_grad.argtypes = [C.c_int, FP, FP, FP, FP, C.c_float, FP, FP, FP, C.c_int, C.c_int, FP, FP, FP, C.c_float, C.c_float, C.c_int, C.c_int,
                                 FP, FP] + [FP] * 9
    return h


def host_grads(h, s, kw, w):
    cam = s["cam"]
    n, W, H = len(s["means"]), cam["W"], cam["H"]
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    cov6, shs = f32(kw.get("cov6")), f32(kw.get("shs"))
    sh_k = 0 if shs is None else shs.shape[1]
    out = dict(color=np.zeros((3, H, W), np.float32), means3D=np.zeros((n, 3), np.float32), means2D=np.zeros((n, 3), np.float32),
               opacities=np.zeros(n, np.float32), colors=np.zeros((n, 3), np.float32), shs=np.zeros((n, max(sh_k, 1), 3), np.float32),
               cov3D=np.zeros((n, 6), np.float32), scales=np.zeros((n, 3), np.float32), rotations=np.zeros((n, 4), np.float32))
    keep = [f32(s["means"]), f32(s["scales"]), f32(s["rotations"]), f32(np.asarray(s["opacity"]).reshape(-1)), f32(s["colors"]),
            f32(cam["campos"]), f32(cam["V"]).reshape(16), f32(cam["P"]).reshape(16), f32(s["bg"]), f32(w)]
    reach = h.hh_raster_grad(n, fp(keep[0]), fp(cov6), None if cov6 is not None else fp(keep[1]), None if cov6 is not None else fp(keep[2]),
                             float(s["scale_modifier"]), fp(keep[3]), None if shs is not None else fp(keep[4]), fp(shs), sh_k, int(kw.get("sh_degree", 0)),
                             fp(keep[5]), fp(keep[6]), fp(keep[7]), cam["tanfovx"], cam["tanfovy"], W, H, fp(keep[8]), fp(keep[9]),
                             *[fp(out[k]) for k in ("color", "means3D", "means2D", "opacities", "colors", "shs", "cov3D", "scales", "rotations")])
    return out, reach


CASES = [("e", "cov", None), ("g", "cov", None), ("w", "cov", None), ("w", "sr", 3), ("small", "sr", 0), ("small", "sr", 1), ("small", "sr", 2),
         ("small", "cov", 3)]


@pytest.mark.parametrize("name,form,degree", CASES)
def test_header_gradients_against_the_float64_oracle(host, name, form, degree):
    s, kw, w, share, r64, y = gr.reference(name, form, degree)
    assert share <= gr.MAX_ZERO_SHARE, f"{name}: {share:.4f} of the pixels are borderline: the scene is not fit to compare on"
    got, reach = host_grads(host, s, kw, w)
    K = r64["n_contrib_max"]
    assert reach == K
    contributes = np.abs(r64["grads"]["opacities"]) > 0
    if name in ("w", "small"):
        assert (r64["clamped"] & contributes).any(), "the 1.3 tanfov clamp is active on no contributing Gaussian"
    if degree is not None:
        assert (r64["sh_clamped"] & contributes[:, None]).any() and (~r64["sh_clamped"] & contributes[:, None]).any(), "the SH zero clamp"
    assert (~r64["valid"]).sum() == 0 or all(np.all(got[q][~r64["valid"]] == 0) for q in r64["grads"]), "a culled Gaussian has a gradient"
    for q, ref in r64["grads"].items():
        if q == "colors" and degree is not None:
            continue
        err = gr.rel_l2(got[q].reshape(ref.shape), ref)
        print(f"scene {name} {form} sh {degree}: {q}: y {y[q]:.3e}, header error {err:.3e} = {err / y[q] if y[q] > 0 else 0.0:.2f} y, K {K}")
        assert err <= gr.bar(y[q], K), f"{name} {q}: error {err:.3e} exceeds 3 y + 2 K 2^-24 = {gr.bar(y[q], K):.3e}"
