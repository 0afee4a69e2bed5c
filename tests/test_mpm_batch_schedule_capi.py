"""CPU checks of the per-scene schedule entry point of the batch ABI (pixie_mpm_batch_run, struct pixie_batch_sched): declared in the
product section of include/pixie_hip.h, typed in _lib.SIGNATURES, exported by both libraries, laid out as gcc lays out the header, and
refusing null arguments without touching a device."""
import ctypes as C
import os
import re
import subprocess

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pixie_hip.h")


def product_section():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    head, sep, tail = text.partition("#ifdef PIXIE_DIAG")
    assert sep
    return head + tail.partition("#endif")[2]


def defined_symbols(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {l.split()[-1] for l in out.splitlines()}


def test_header_declares_batch_run_in_the_product_section():
    prod = product_section()
    assert re.search(r"\bint\s+pixie_mpm_batch_run\s*\(\s*pixie_mpm_batch\s*\*\s*\w+\s*,\s*const\s+pixie_batch_sched\s*\*", prod)
    assert "typedef struct pixie_batch_sched" in prod
    assert "1 ... 32 distinct handles (kMaxBatch)" in open(HEADER).read()


def test_signature_and_both_libraries_export_it():
    assert "pixie_mpm_batch_run" in _lib.SIGNATURES and "pixie_mpm_batch_run" not in _lib.DIAG_SIGNATURES
    res, args = _lib.SIGNATURES["pixie_mpm_batch_run"]
    assert res is C.c_int and len(args) == 4 and args[1] is C.POINTER(_lib.BatchSched)
    _lib.load(), _lib.load(diag=True)
    assert "pixie_mpm_batch_run" in defined_symbols(_lib.LIB_PATH)
    assert "pixie_mpm_batch_run" in defined_symbols(_lib.DIAG_LIB_PATH)


def test_sched_struct_layout_matches_header(tmp_path):
    cls, cname = _lib.BatchSched, "pixie_batch_sched"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ["return 0; }"]
    src = tmp_path / "sched_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sched_layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    # every field of the header's struct is mirrored (names in declaration order)
    body = re.search(r"typedef struct pixie_batch_sched \{(.*?)\} pixie_batch_sched;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        rest = decl.split(None, 1)[1]
        declared += [re.sub(r"\[.*", "", p.strip().lstrip("*").strip()) for p in rest.split(",")]
    assert declared == [f for f, _ in cls._fields_]


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    sched = (_lib.BatchSched * 2)()
    assert lib.pixie_mpm_batch_run(None, sched, 2, None) != 0
    assert b"null argument" in lib.pixie_last_error()
    b = C.c_void_p()
    assert lib.pixie_mpm_batch_create(C.byref(b), None, 2) != 0     # (no batch can be created without handles)
    assert not b.value
    assert lib.pixie_mpm_batch_run(b, None, 0, None) != 0
    assert b"null argument" in lib.pixie_last_error()
