"""CPU checks of the multi-scene MPM entry points (pixie_mpm_batch_*): declared in the product section of include/pixie_hip.h,
typed in _lib.SIGNATURES, exported by both libraries, and refusing bad handle lists before touching a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ("pixie_mpm_batch_create", "pixie_mpm_batch_step", "pixie_mpm_batch_destroy")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pixie_hip.h")).read(), flags=re.S)


def test_header_declares_the_batch_entry_points_outside_the_diag_section():
    text = _header()
    product, sep, tail = text.partition("#ifdef PIXIE_DIAG")
    assert sep
    diag_part = tail.partition("#endif")[0]
    for nm in BATCH:
        assert re.search(r"\b" + nm + r"\s*\(", product), nm
        assert nm not in diag_part, nm
    assert "typedef struct pixie_mpm_batch pixie_mpm_batch;" in product
    # the limit is stated in the header
    assert re.search(r"1 \.\.\. 32 distinct handles \(kMaxBatch\)", open(os.path.join(REPO, "include", "pixie_hip.h")).read())


def test_signatures_and_both_libraries_export_them():
    for nm in BATCH:
        assert nm in _lib.SIGNATURES, nm
        assert nm not in _lib.DIAG_SIGNATURES, nm
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        names = {l.split()[-1] for l in out.splitlines()}
        for nm in BATCH:
            assert nm in names, (path, nm)


@pytest.mark.parametrize("diag", [False, True])
def test_create_refuses_bad_lists_without_a_device(diag):
    lib = _lib.load(diag=diag)
    out = C.c_void_p(123)
    # null list
    assert lib.pixie_mpm_batch_create(C.byref(out), None, 1) != 0
    assert b"null" in lib.pixie_last_error()
    assert out.value is None
    # empty list
    arr = (C.c_void_p * 1)(None)
    assert lib.pixie_mpm_batch_create(C.byref(out), arr, 0) != 0
    assert b"32" in lib.pixie_last_error()
    # longer than kMaxBatch (the entries are never dereferenced: the length is checked first)
    arr = (C.c_void_p * 33)(*([C.c_void_p(0x1000 + 64 * i) for i in range(33)]))
    assert lib.pixie_mpm_batch_create(C.byref(out), arr, 33) != 0
    assert b"32" in lib.pixie_last_error()
    # a null handle in the list
    arr = (C.c_void_p * 2)(None, None)
    assert lib.pixie_mpm_batch_create(C.byref(out), arr, 2) != 0
    assert b"null handle" in lib.pixie_last_error()
    # a handle listed twice (found before any handle is dereferenced)
    arr = (C.c_void_p * 2)(C.c_void_p(0x1000), C.c_void_p(0x1000))
    assert lib.pixie_mpm_batch_create(C.byref(out), arr, 2) != 0
    assert b"same handle" in lib.pixie_last_error()
    # step / destroy of nothing
    assert lib.pixie_mpm_batch_step(None, 1e-4, 1, None) != 0
    assert lib.pixie_mpm_batch_destroy(None) == 0
