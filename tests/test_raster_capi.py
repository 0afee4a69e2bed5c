"""CPU checks of the rasteriser's boundary: the entry points of section D of include/pixie_hip.h are declared, typed and exported,
struct pixie_raster_desc is laid out as gcc lays it out, pixie_amd/rasterizer.py mirrors the reference's interface (field order, the
two argument errors) and refuses to compute without a device."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pixie_hip.h")
NAMES = ("pixie_raster_workspace_bytes", "pixie_raster_forward", "pixie_sh_to_rgb")


def settings(device="cpu", W=32, H=24):
    from pixie_amd.rasterizer import GaussianRasterizationSettings
    eye = torch.eye(4, device=device)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3, device=device),
                                         scale_modifier=1.0, viewmatrix=eye, projmatrix=eye, sh_degree=0,
                                         campos=torch.zeros(3, device=device), prefiltered=False, debug=False)


def test_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prod = text.partition("#ifdef PIXIE_DIAG")[0]
    syms = lambda p: {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", p], text=True).splitlines()}
    for nm in NAMES:
        assert re.search(r"\b" + nm + r"\s*\(", prod), nm
        assert nm in _lib.SIGNATURES and nm not in _lib.DIAG_SIGNATURES
        assert nm in syms(_lib.LIB_PATH) and nm in syms(_lib.DIAG_LIB_PATH)
    assert _lib.SIGNATURES["pixie_raster_workspace_bytes"] == (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64])
    res, args = _lib.SIGNATURES["pixie_raster_forward"]
    assert res is C.c_int and args[0] is C.POINTER(_lib.RasterDesc) and args[1] is C.POINTER(C.c_int64) and len(args) == 3
    assert len(_lib.SIGNATURES["pixie_sh_to_rgb"][1]) == 10


def test_raster_desc_layout_matches_header(tmp_path):
    cls, cname = _lib.RasterDesc, "pixie_raster_desc"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {", f'printf("sizeof %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ["return 0; }"]
    src = tmp_path / "raster_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "raster_layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    body = re.search(r"typedef struct pixie_raster_desc \{(.*?)\} pixie_raster_desc;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        names = decl.rsplit(None, 1)[1] if "," not in decl else decl.split(None, 1)[1]
        declared += [re.sub(r"\[.*", "", nm.strip().lstrip("*")) for nm in names.split(",")]
    assert declared == [f for f, _ in cls._fields_]


def test_settings_have_the_reference_field_order():
    from pixie_amd.rasterizer import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                                                     "projmatrix", "sh_degree", "campos", "prefiltered", "debug")


def test_argument_combination_errors():
    from pixie_amd.rasterizer import GaussianRasterizer
    r = GaussianRasterizer(settings())
    m, o, c, sh = torch.zeros(4, 3), torch.ones(4, 1), torch.ones(4, 3), torch.zeros(4, 1, 3)
    cov, sc, rot = torch.zeros(4, 6), torch.ones(4, 3), torch.ones(4, 4)
    msg1 = "Please provide excatly one of either SHs or precomputed colors!"
    msg2 = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
    for kw in (dict(cov3D_precomp=cov), dict(shs=sh, colors_precomp=c, cov3D_precomp=cov)):
        with pytest.raises(Exception) as e:
            r(m, None, o, **kw)
        assert str(e.value) == msg1
    for kw in (dict(colors_precomp=c), dict(colors_precomp=c, scales=sc), dict(colors_precomp=c, rotations=rot),
               dict(colors_precomp=c, scales=sc, rotations=rot, cov3D_precomp=cov), dict(colors_precomp=c, scales=sc, cov3D_precomp=cov)):
        with pytest.raises(Exception) as e:
            r(m, None, o, **kw)
        assert str(e.value) == msg2
    import inspect
    assert list(inspect.signature(r.forward).parameters)[:8] == ["means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                                                                 "cov3D_precomp"]


def test_bad_arguments_are_refused_by_the_library():
    lib = _lib.load()
    assert lib.pixie_raster_forward(None, None, None) != 0 and b"null descriptor" in lib.pixie_last_error()
    d = _lib.RasterDesc()
    d.n, d.width, d.height = -1, 8, 8
    assert lib.pixie_raster_forward(C.byref(d), None, None) != 0 and b"< 0" in lib.pixie_last_error()
    d.n, d.width = 0, 0
    assert lib.pixie_raster_forward(C.byref(d), None, None) != 0 and b"must be positive" in lib.pixie_last_error()
    assert lib.pixie_raster_workspace_bytes(4, 0, 8, 16) == -1 and b"must be positive" in lib.pixie_last_error()
    assert lib.pixie_raster_workspace_bytes(4, 8, 8, -1) == -1 and b"max_instances" in lib.pixie_last_error()
    cam = (C.c_float * 3)()
    assert lib.pixie_sh_to_rgb(None, -1, 1, 0, None, cam, None, 0, None, None) != 0 and b"< 0" in lib.pixie_last_error()
    assert lib.pixie_sh_to_rgb(None, 4, 1, 1, None, cam, None, 0, None, None) != 0 and b"fewer" in lib.pixie_last_error()
    assert lib.pixie_sh_to_rgb(None, 4, 16, 4, None, cam, None, 0, None, None) != 0 and b"outside 0..3" in lib.pixie_last_error()
    assert lib.pixie_sh_to_rgb(None, 4, 16, 3, None, cam, None, 0, None, None) != 0 and b"null pointer" in lib.pixie_last_error()
    assert lib.pixie_sh_to_rgb(None, 0, 16, 3, None, cam, None, 0, None, None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device failure mode")
def test_every_entry_point_raises_without_a_device():
    from types import SimpleNamespace
    from pixie_amd import rasterizer as R
    r = R.GaussianRasterizer(settings())
    m, o, c, cov = torch.zeros(4, 3), torch.ones(4, 1), torch.ones(4, 3), torch.zeros(4, 6)
    with pytest.raises(ValueError, match="no CPU path"):
        r(m, None, o, colors_precomp=c, cov3D_precomp=cov)
    with pytest.raises(ValueError, match="no CPU path"):
        r(m, None, o, shs=torch.zeros(4, 1, 3), scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(ValueError, match="no CPU path"):
        R.sh_to_rgb(torch.zeros(4, 16, 3), 3, m, torch.zeros(3))
    cam, pc = SimpleNamespace(camera_center=torch.zeros(3)), SimpleNamespace(max_sh_degree=3, active_sh_degree=3)
    with pytest.raises(ValueError, match="no CPU path"):
        R.convert_SH(torch.zeros(4, 16, 3), cam, pc, m)
    with pytest.raises(ValueError, match="no CPU path"):
        R.render_frames((torch.zeros(2, 4, 3), torch.zeros(2, 4, 6)), settings(), o, colors_precomp=c)
    # the library itself: a render cannot size its workspace or launch without a device
    lib = _lib.load()
    d = _lib.RasterDesc()
    d.n, d.width, d.height, d.tanfovx, d.tanfovy = 0, 8, 8, 1.0, 1.0
    d.d_out_color = 16
    assert lib.pixie_raster_forward(C.byref(d), None, None) != 0
    assert lib.pixie_last_error()
