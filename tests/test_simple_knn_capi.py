"""CPU checks of the C ABI of distCUDA2 and of the fused photometric loss (include/pixie_hip.h): the size queries and the refusals,
all of which return before anything is launched, so they need no device."""
import ctypes as C

from pixie_amd import _lib

NAMES = ("pixie_knn_mean_dist2_scratch_bytes", "pixie_knn_mean_dist2", "pixie_photometric_workspace_bytes",
         "pixie_photometric_forward", "pixie_photometric_backward")
FAKE = C.c_void_p(0x1000)            # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused first


def test_symbols_are_declared_and_typed():
    lib = _lib.load()
    for nm in NAMES:
        assert nm in _lib.SIGNATURES and hasattr(lib, nm)
    assert _lib.SIGNATURES["pixie_knn_mean_dist2"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])


def test_knn_scratch_query_is_monotone():
    lib = _lib.load()
    ladder = [0, 1, 3, 4, 63, 64, 65, 1000, 1023, 1024, 1025, 4096, 10 ** 5, 10 ** 5 + 1, 10 ** 6, 3 * 10 ** 6, 2 ** 24 - 1, 2 ** 24]
    sizes = [lib.pixie_knn_mean_dist2_scratch_bytes(n) for n in ladder]
    assert all(s >= 0 for s in sizes), sizes
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), list(zip(ladder, sizes))
    assert sizes[1] > 0 and sizes[-1] >= 2 ** 24 * (4 * 4 + 16)          # four index / code arrays and the gathered points
    assert lib.pixie_knn_mean_dist2_scratch_bytes(-1) == -1 and b"2^24" in lib.pixie_last_error()
    assert lib.pixie_knn_mean_dist2_scratch_bytes(2 ** 24 + 1) == -1 and b"2^24" in lib.pixie_last_error()


def test_knn_refusals_launch_nothing():
    lib = _lib.load()
    assert lib.pixie_knn_mean_dist2(FAKE, 2 ** 24 + 1, FAKE, 1 << 40, FAKE, None) != 0
    assert b"2^24" in lib.pixie_last_error()
    assert lib.pixie_knn_mean_dist2(FAKE, -1, FAKE, 1 << 40, FAKE, None) != 0 and b"< 0" in lib.pixie_last_error()
    need = lib.pixie_knn_mean_dist2_scratch_bytes(1000)
    assert lib.pixie_knn_mean_dist2(FAKE, 1000, FAKE, need - 1, FAKE, None) != 0
    assert b"smaller than" in lib.pixie_last_error() and str(need).encode() in lib.pixie_last_error()
    assert lib.pixie_knn_mean_dist2(FAKE, 1000, None, need, FAKE, None) != 0 and b"smaller than" in lib.pixie_last_error()
    assert lib.pixie_knn_mean_dist2(None, 1000, FAKE, need, FAKE, None) != 0 and b"null pointer" in lib.pixie_last_error()
    assert lib.pixie_knn_mean_dist2(FAKE, 1000, C.c_void_p(0x1004), need, FAKE, None) != 0 and b"aligned" in lib.pixie_last_error()
    assert lib.pixie_knn_mean_dist2(None, 0, None, 0, None, None) == 0            # nothing to do, nothing launched


def test_photometric_size_query_and_refusals():
    lib = _lib.load()
    tiles = lambda h, w: ((h + 15) // 16) * ((w + 15) // 16)
    for b, c, h, w in ((1, 3, 1, 1), (1, 3, 37, 53), (2, 3, 20, 24), (1, 3, 800, 800)):
        plain = lib.pixie_photometric_workspace_bytes(b, c, h, w, 0)
        grad = lib.pixie_photometric_workspace_bytes(b, c, h, w, 1)
        assert plain >= 8 * b * c * tiles(h, w) and grad - plain == 3 * 4 * b * c * h * w
    assert lib.pixie_photometric_workspace_bytes(1, 3, 0, 8, 1) == -1 and b"positive" in lib.pixie_last_error()
    assert lib.pixie_photometric_workspace_bytes(1, 0, 8, 8, 1) == -1 and b"positive" in lib.pixie_last_error()
    assert lib.pixie_photometric_workspace_bytes(1, 3, 40000, 8, 0) == -1 and b"32768" in lib.pixie_last_error()
    assert lib.pixie_photometric_workspace_bytes(30000, 3, 8, 8, 0) == -1 and b"65535" in lib.pixie_last_error()
    need = lib.pixie_photometric_workspace_bytes(1, 3, 37, 53, 1)
    assert lib.pixie_photometric_forward(FAKE, FAKE, 1, 3, 37, 53, FAKE, need - 1, 1, FAKE, FAKE, None) != 0
    assert b"smaller than" in lib.pixie_last_error()
    assert lib.pixie_photometric_forward(None, FAKE, 1, 3, 37, 53, FAKE, need, 1, FAKE, FAKE, None) != 0 and b"null pointer" in lib.pixie_last_error()
    assert lib.pixie_photometric_backward(FAKE, FAKE, 1, 3, 37, 53, None, FAKE, FAKE, FAKE, None) != 0 and b"null pointer" in lib.pixie_last_error()
    assert lib.pixie_photometric_backward(FAKE, FAKE, 1, 3, 0, 53, FAKE, FAKE, FAKE, FAKE, None) != 0 and b"positive" in lib.pixie_last_error()
