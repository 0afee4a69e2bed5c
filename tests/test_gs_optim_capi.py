"""CPU check of the training-step natives' C boundary: sizeof / offsetof of every struct field, as gcc lays out
include/pixie_hip.h, equal the ctypes mirrors in pixie_amd/_lib.py, and the argument checks that need no device."""
import ctypes as C
import os
import subprocess

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"pixie_gs_adam_group": _lib.GsAdamGroup, "pixie_gs_adam_desc": _lib.GsAdamDesc, "pixie_gs_densify_desc": _lib.GsDensifyDesc,
           "pixie_gs_densify_outs": _lib.GsDensifyOuts}


def test_struct_layouts_match_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "pixie_hip.h")}"', "int main(void) {"]
    for cname, cls in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_argument_checks_come_before_any_launch():
    lib = _lib.load()
    desc = _lib.GsAdamDesc()
    desc.n_groups = 9
    assert lib.pixie_gs_adam_step(C.byref(desc), None) != 0 and b"n_groups" in lib.pixie_last_error()
    desc.n_groups = 3                                         # three empty groups: legal, nothing to launch
    assert lib.pixie_gs_adam_step(C.byref(desc), None) == 0
    desc.group[1].count = 4                                   # a non-empty group needs its pointers
    assert lib.pixie_gs_adam_step(C.byref(desc), None) != 0 and b"null pointer" in lib.pixie_last_error()
    assert lib.pixie_gs_densify_stats(None, None, 0, None, None, None, None) == 0
    assert lib.pixie_gs_densify_stats(None, None, 5, None, None, None, None) != 0
    d = _lib.GsDensifyDesc()
    counts, n_split = (C.c_int64 * 4)(), (C.c_int64 * 1)()
    d.n, d.max_grad = 10, 0.0
    assert lib.pixie_gs_densify_plan(C.byref(d), counts, n_split, None) == _lib.GS_DENSIFY_BAD_MAX_GRAD
    d.max_grad = float("nan")
    assert lib.pixie_gs_densify_plan(C.byref(d), counts, n_split, None) == _lib.GS_DENSIFY_BAD_MAX_GRAD
    d.n, d.max_grad = 2 ** 31 - 1, 2e-4
    assert lib.pixie_gs_densify_plan(C.byref(d), counts, n_split, None) == _lib.GS_DENSIFY_TOO_MANY_ROWS
    d.n = 0
    assert lib.pixie_gs_densify_plan(C.byref(d), counts, n_split, None) == _lib.GS_DENSIFY_EMPTY
    assert lib.pixie_gs_densify_emit(C.byref(d), None, None) == _lib.GS_DENSIFY_EMPTY
    assert lib.pixie_gs_densify_workspace_bytes(-1) == -1
