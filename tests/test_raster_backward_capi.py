"""CPU checks of the boundary of the rasteriser's backward pass (include/pixie_hip.h, section D'): the entry points are declared, typed
and exported, struct pixie_raster_backward_desc is laid out as gcc lays it out, and every argument error is refused with a message
that names the field before anything is launched or written (the pointers below are never dereferenced: they point nowhere)."""
import ctypes as C
import os
import re
import subprocess

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pixie_hip.h")
NAMES = ("pixie_raster_backward_workspace_bytes", "pixie_raster_backward")
FAKE = 1 << 20              # a 16-byte aligned address that is never read or written


def desc(form="cov", n=8, instances=32):
    b = _lib.RasterBackwardDesc()
    f = b.forward
    f.n, f.width, f.height, f.tanfovx, f.tanfovy, f.scale_modifier = n, 32, 24, 0.5, 0.4, 1.0
    for name in ("d_means", "d_colors", "d_opacity", "d_out_color", "d_radii", "d_final_T", "d_n_contrib", "d_workspace"):
        setattr(f, name, FAKE)
    f.workspace_bytes = 1 << 30
    if form == "cov":
        f.d_cov3d = FAKE
    else:
        f.d_scales = f.d_rotations = FAKE
    b.instances = instances
    b.d_dL_dcolor = FAKE
    b.d_grad_workspace, b.grad_workspace_bytes = FAKE, 1 << 30
    b.d_dL_dopacity = FAKE
    return b


def refused(b, *words):
    lib = _lib.load()
    rc = lib.pixie_raster_backward(C.byref(b), None)
    msg = lib.pixie_last_error().decode()
    assert rc != 0, "accepted"
    for w in words:
        assert w in msg, (w, msg)


def test_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prod = text.partition("#ifdef PIXIE_DIAG")[0]
    syms = lambda p: {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", p], text=True).splitlines()}
    for nm in NAMES:
        assert re.search(r"\b" + nm + r"\s*\(", prod), nm
        assert nm in _lib.SIGNATURES and nm not in _lib.DIAG_SIGNATURES
        assert nm in syms(_lib.LIB_PATH) and nm in syms(_lib.DIAG_LIB_PATH)
    assert _lib.SIGNATURES["pixie_raster_backward_workspace_bytes"] == (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64])
    res, args = _lib.SIGNATURES["pixie_raster_backward"]
    assert res is C.c_int and args[0] is C.POINTER(_lib.RasterBackwardDesc) and len(args) == 2


def test_backward_desc_layout_matches_header(tmp_path):
    cls, cname = _lib.RasterBackwardDesc, "pixie_raster_backward_desc"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {", f'printf("sizeof %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ["return 0; }"]
    src = tmp_path / "raster_backward_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "raster_backward_layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_workspace_bytes():
    lib = _lib.load()
    assert lib.pixie_raster_backward_workspace_bytes(8, 32, 24, 0) == 0
    assert lib.pixie_raster_backward_workspace_bytes(8, 32, 24, 100) >= 100 * 9 * 4
    assert lib.pixie_raster_backward_workspace_bytes(8, 32, 24, -1) == -1 and b"instances" in lib.pixie_last_error()
    assert lib.pixie_raster_backward_workspace_bytes(8, 0, 24, 4) == -1 and b"image" in lib.pixie_last_error()


def test_missing_forward_outputs_are_refused():
    assert _lib.load().pixie_raster_backward(None, None) != 0
    b = desc()
    b.forward.d_final_T = None
    refused(b, "d_final_T")
    b = desc()
    b.forward.d_n_contrib = None
    refused(b, "d_n_contrib")
    b = desc()
    b.d_dL_dcolor = None
    refused(b, "d_dL_dcolor")


def test_small_gradient_workspace_is_refused():
    b = desc(instances=1000)
    b.grad_workspace_bytes = 1000 * 9 * 4 - 1
    refused(b, "d_grad_workspace", "1000 instances")
    b = desc(instances=1000)
    b.d_grad_workspace = None
    refused(b, "d_grad_workspace")


def test_covariance_gradient_form_must_match_the_forward():
    b = desc("cov")
    b.d_dL_dscales = FAKE
    refused(b, "d_dL_dscales", "d_cov3d")
    b = desc("cov")
    b.d_dL_drotations = FAKE
    refused(b, "d_dL_drotations", "d_cov3d")
    b = desc("sr")
    b.d_dL_dcov3D = FAKE
    refused(b, "d_dL_dcov3D", "d_scales")
    for form in ("cov", "sr"):                 # both forms at once
        b = desc(form)
        b.d_dL_dcov3D = b.d_dL_dscales = b.d_dL_drotations = FAKE
        refused(b, "d_dL_dcov3D", "d_dL_dscales", "not both")


def test_sh_arguments_are_checked():
    b = desc()
    b.d_shs, b.sh_k = FAKE, 16
    for degree in (-1, 4):
        b.sh_degree = degree
        refused(b, "sh_degree", "outside 0..3")
    for degree, k in ((1, 3), (2, 8), (3, 15)):
        b.sh_degree, b.sh_k = degree, k
        refused(b, "sh_k", "fewer")
    b = desc()
    b.d_dL_dshs = FAKE
    refused(b, "d_dL_dshs", "d_shs")


def test_all_null_outputs_is_a_no_op():
    b = desc()
    b.d_dL_dopacity = None
    lib = _lib.load()
    assert lib.pixie_raster_backward(C.byref(b), None) == 0
    b = desc("sr")
    b.d_dL_dopacity = None
    b.d_shs, b.sh_k, b.sh_degree = FAKE, 16, 3
    assert lib.pixie_raster_backward(C.byref(b), None) == 0
