"""CPU checks of the splat entry points of the C ABI (pixie_splat_from_cov, pixie_mpm_export_frame_splats,
pixie_mpm_batch_run_splats, struct pixie_batch_splat_out): declared in the product section of include/pixie_hip.h, typed in
_lib.SIGNATURES, exported by both libraries, laid out as gcc lays out the header, and refusing bad arguments without a device."""
import ctypes as C
import os
import re
import subprocess

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pixie_hip.h")
NAMES = ("pixie_splat_from_cov", "pixie_mpm_export_frame_splats", "pixie_mpm_batch_run_splats")


def product_section():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    head, sep, tail = text.partition("#ifdef PIXIE_DIAG")
    assert sep
    return head + tail.partition("#endif")[2]


def defined_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {l.split()[-1] for l in out.splitlines()}


def test_declared_typed_and_exported():
    prod = product_section()
    for nm in NAMES:
        assert re.search(r"\bint\s+" + nm + r"\s*\(", prod), nm
        assert nm in _lib.SIGNATURES and nm not in _lib.DIAG_SIGNATURES, nm
        assert nm in defined_symbols(_lib.LIB_PATH) and nm in defined_symbols(_lib.DIAG_LIB_PATH), nm
    assert "typedef struct pixie_batch_splat_out" in prod
    res, args = _lib.SIGNATURES["pixie_mpm_batch_run_splats"]
    assert res is C.c_int and args[1] is C.POINTER(_lib.BatchSched) and args[2] is C.POINTER(_lib.BatchSplatOut) and len(args) == 5
    assert _lib.SIGNATURES["pixie_splat_from_cov"][1][1] is C.c_int64
    assert len(_lib.SIGNATURES["pixie_mpm_export_frame_splats"][1]) == 11


def test_splat_out_struct_layout_matches_header(tmp_path):
    cls, cname = _lib.BatchSplatOut, "pixie_batch_splat_out"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ["return 0; }"]
    src = tmp_path / "splat_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "splat_layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    body = re.search(r"typedef struct pixie_batch_splat_out \{(.*?)\} pixie_batch_splat_out;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"\[.*", "", d.strip().split(None, 1)[1].lstrip("*").strip()) for d in body.split(";") if d.strip()]
    assert declared == [f for f, _ in cls._fields_]


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.pixie_splat_from_cov(None, -1, None, None, None) != 0
    assert b"< 0" in lib.pixie_last_error()
    assert lib.pixie_splat_from_cov(None, 4, None, None, None) != 0
    assert b"null pointer" in lib.pixie_last_error()
    assert lib.pixie_splat_from_cov(None, 0, None, None, None) == 0          # nothing to do
    d3 = (C.c_double * 3)()
    assert lib.pixie_mpm_export_frame_splats(None, 1, d3, 1.0, d3, (C.c_double * 9)(), None, None, None, None, None) != 0
    assert b"null argument" in lib.pixie_last_error()
    assert lib.pixie_mpm_batch_run_splats(None, (_lib.BatchSched * 1)(), None, 1, None) != 0
    assert b"null argument" in lib.pixie_last_error()
