"""CPU checks of the batched rasteriser's boundary: the three names section D of include/pixie_hip.h gains are declared in its
production part, typed and exported by both libraries, struct pixie_raster_batch_desc and struct pixie_raster_view are laid out as
gcc lays them out, the library reports its limits, and pixie_amd/rasterizer.py refuses what it cannot render (host tensors, both or
neither colour source, a settings list of the wrong length)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pixie_hip.h")
NAMES = ("pixie_raster_batch_workspace_bytes", "pixie_raster_forward_batch")
STRUCTS = {"pixie_raster_batch_desc": "RasterBatchDesc", "pixie_raster_view": "RasterView"}
MSG = "Please provide excatly one of either SHs or precomputed colors!"


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
    assert re.search(r"\}\s*pixie_raster_batch_desc\s*;", prod) and re.search(r"\}\s*pixie_raster_view\s*;", prod)
    assert _lib.SIGNATURES["pixie_raster_batch_workspace_bytes"] == (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64])
    res, args = _lib.SIGNATURES["pixie_raster_forward_batch"]
    assert res is C.c_int and args[0] is C.POINTER(_lib.RasterBatchDesc) and args[1] is C.POINTER(C.c_int64)
    assert args[2] is C.POINTER(C.c_int32) and len(args) == 4
    # the single-view entry points are as they were
    assert _lib.SIGNATURES["pixie_raster_workspace_bytes"] == (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64])
    assert len(_lib.SIGNATURES["pixie_raster_forward"][1]) == 3 and len(_lib.SIGNATURES["pixie_sh_to_rgb"][1]) == 10


def declared_fields(cname):
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        decl = re.sub(r"^(const\s+)?\w+\s*\**\s*", "", decl)            # drop the type of the declaration
        out += [re.sub(r"\[.*", "", nm.strip().lstrip("*").strip()) for nm in decl.split(",")]
    return out


def test_struct_layouts_match_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in getattr(_lib, pyname)._fields_]
    lines += ["return 0; }"]
    src = tmp_path / "raster_batch_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "raster_batch_layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, pyname in STRUCTS.items():
        cls = getattr(_lib, pyname)
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
        assert declared_fields(cname) == [f for f, _ in cls._fields_], cname
    assert C.sizeof(_lib.RasterView) == 37 * 4


def test_bad_arguments_are_refused_by_the_library():
    lib = _lib.load()
    err = lambda: lib.pixie_last_error()
    assert lib.pixie_raster_forward_batch(None, None, None, None) != 0 and b"null descriptor" in err()
    d = _lib.RasterBatchDesc()
    d.views, d.n_dyn, d.n_static, d.width, d.height = 2, -1, 0, 8, 8
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b">= 0" in err()
    d.n_dyn, d.views = 4, 0
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"1..65535" in err()
    d.views = 65536
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"1..65535" in err()
    d.views, d.n_dyn = 65535, 40000                                   # 65535 x 40000 > 2^31 - 1
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"one scan" in err()
    d.views, d.n_dyn, d.width = 2, 4, 0
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"must be positive" in err()
    d.width, d.max_instances = 8, 1 << 32
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"max_instances" in err()
    d.max_instances = 64
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"per-view cameras" in err()
    views = (_lib.RasterView * 2)()
    d.view = views
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"must be positive" in err()
    for v in views:
        v.tanfovx = v.tanfovy = 0.5
    counts, groups = (C.c_int64 * 2)(5, 5), C.c_int32(9)
    assert lib.pixie_raster_forward_batch(C.byref(d), counts, C.byref(groups), None) != 0 and b"d_out_color and d_out_rgb8" in err()
    assert list(counts) == [0, 0] and groups.value == 0
    d.d_out_rgb8 = 16
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"d_means and d_cov3d" in err()
    d.d_means = d.d_cov3d = 16
    d.n_static = 3
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"d_static_means and d_static_cov3d" in err()
    d.d_static_means = d.d_static_cov3d = d.d_opacity = 16
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"exactly one of d_colors and d_shs" in err()
    d.d_colors = d.d_shs = 16
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"exactly one of d_colors and d_shs" in err()
    d.d_colors, d.sh_degree, d.k_coeffs = None, 2, 4
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"fewer" in err()
    d.sh_degree = 4
    assert lib.pixie_raster_forward_batch(C.byref(d), None, None, None) != 0 and b"outside 0..3" in err()
    assert lib.pixie_raster_batch_workspace_bytes(4, 0, 8, 8, 16) == -1 and b"1..65535" in err()
    assert lib.pixie_raster_batch_workspace_bytes(4, 2, 0, 8, 16) == -1 and b"must be positive" in err()
    assert lib.pixie_raster_batch_workspace_bytes(4, 2, 8, 8, -1) == -1 and b"max_instances" in err()
    assert lib.pixie_raster_batch_workspace_bytes(40000, 65535, 8, 8, 16) == -1 and b"one scan" in err()


def test_argument_errors_of_the_python_layer():
    from pixie_amd import rasterizer as R
    F, n = 3, 4
    frames = (torch.zeros(F, n, 3), torch.zeros(F, n, 6))
    o, c, sh = torch.ones(n), torch.ones(n, 3), torch.zeros(n, 1, 3)
    for fn in (lambda **kw: R.render_frame_batch(frames, settings(), o, **kw),
               lambda **kw: R.FrameBatchRasterizer()(frames[0], frames[1], settings(), o, **kw),
               lambda **kw: R.render_frames(frames, settings(), o, batch=True, **kw)):
        for kw in (dict(), dict(shs=sh, colors_precomp=c)):
            with pytest.raises(Exception) as e:
                fn(**kw)
            assert str(e.value) == MSG
    for count in (2, 4):
        with pytest.raises(ValueError, match=f"{count} settings for 3"):
            R.render_frame_batch(frames, [settings()] * count, o, colors_precomp=c)
        with pytest.raises(ValueError, match=f"{count} settings for 3"):
            R.FrameBatchRasterizer()(frames[0], frames[1], [settings()] * count, o, colors_precomp=c)
    with pytest.raises(ValueError, match="no covariance"):
        R.render_frame_batch((frames[0], None), settings(), o, colors_precomp=c)
    # host tensors: there is no CPU path
    for fn in (lambda: R.render_frame_batch(frames, settings(), o, colors_precomp=c),
               lambda: R.render_frame_batch(frames, [settings()] * F, o, shs=sh, out_rgb8=True),
               lambda: R.render_frames(frames, settings(), o, colors_precomp=c, batch=R.FrameBatchRasterizer()),
               lambda: R.FrameBatchRasterizer()(frames[0], frames[1], settings(), o, colors_precomp=c),
               lambda: R.FrameBatchRasterizer()(frames[0], frames[1], settings(), o, shs=sh, static=(torch.zeros(2, 3), torch.zeros(2, 6)))):
        with pytest.raises(ValueError, match="no CPU path"):
            fn()
    import inspect
    assert list(inspect.signature(R.render_frame_batch).parameters) == ["frames", "settings_per_frame", "opacity", "shs", "colors_precomp", "unselected",
                                                                        "frames_per_call", "out", "out_rgb8", "rasterizer"]
    p = inspect.signature(R.render_frames).parameters
    assert list(p)[:7] == ["frames", "settings_per_frame", "opacity", "shs", "colors_precomp", "unselected", "rasterizer"] and p["batch"].default is None
    assert list(inspect.signature(R.save_frame_pngs).parameters) == ["dir", "rgb8_or_images", "start"]
    r = R.FrameBatchRasterizer()
    assert r.max_workspace_bytes == 1 << 30 and r.last_groups == 0 and r.last_instances == []


def test_default_frames_per_call_bounds_the_fixed_workspace():
    from pixie_amd.rasterizer import _default_frames_per_call
    assert _default_frames_per_call(350_000, 125, 1 << 30) == (1 << 29) // (60 * 350_000)        # 25 frames a call
    assert _default_frames_per_call(5_000, 3, 1 << 30) == 3
    assert _default_frames_per_call(0, 7, 1 << 30) == 7
    assert _default_frames_per_call(10 ** 9, 125, 1 << 40) == 2                                  # views x N stays below 2^31 - 1
    assert _default_frames_per_call(10 ** 6, 125, 1 << 10) == 1
