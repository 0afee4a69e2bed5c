"""GPU checks of pixie_amd.simple_knn.distCUDA2 (pixie_amd/csrc/knn.hip) against tests/_knn_ref.py: the result is BIT-EQUAL to the
float32 brute force in the product's expression order, the same from run to run and under a permutation of the rows.  Sizes
straddle the group of 64 points a wave owns and the 64 groups one ballot bounds (N = 4097 is the first with two rounds).
Input is finite throughout: a NaN coordinate is outside the contract and is not run on a device."""
import numpy as np
import pytest
import torch

from tests import _knn_ref as kr

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
_ref_cache = {}


def cloud(name):
    if name.startswith("uniform"):
        return kr.uniform(int(name[7:]), seed=100 + int(name[7:]))
    return kr.CLOUDS[name]()


def reference(name):
    if name not in _ref_cache:
        _ref_cache[name] = kr.brute32(cloud(name))
    return _ref_cache[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(p, dev):
    from pixie_amd.simple_knn import distCUDA2
    return distCUDA2(torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)).cpu().numpy()


NAMES = [f"uniform{n}" for n in SIZES] + list(kr.CLOUDS)


@pytest.mark.parametrize("name", NAMES)
def test_bit_equal_to_the_float32_brute_force(hip_device, name):
    p = cloud(name)
    got = run(p, hip_device)
    assert got.shape == (len(p),) and got.dtype == np.float32
    ref = reference(name)
    assert np.array_equal(bits(got), bits(ref)), f"{name}: {int((bits(got) != bits(ref)).sum())} of {len(p)} differ"
    if name == "coincident":
        assert np.all(got == 0.0)
    if name in ("uniform1", "uniform3"):                 # FLT_MAX for each missing neighbour: one point overflows, three do not
        assert np.all(np.isposinf(got)) if len(p) == 1 else np.array_equal(bits(got), bits(np.full(3, kr.FLT_MAX / np.float32(3), np.float32)))


def test_two_points_give_inf(hip_device):
    assert np.all(np.isposinf(run(kr.uniform(2, 7), hip_device)))


@pytest.mark.parametrize("name", ["uniform2049", "clustered", "duplicated"])
def test_repeatable_and_permutation_invariant(hip_device, name):
    p = cloud(name)
    a, b = run(p, hip_device), run(p, hip_device)
    assert np.array_equal(bits(a), bits(b))
    perm = np.random.default_rng(9).permutation(len(p))
    assert np.array_equal(bits(run(p[perm], hip_device)), bits(a[perm]))


def test_writes_n_values_and_no_more(hip_device):
    """the C entry point writes into a NaN-filled buffer with a canary tail: every one of the n values is written, the tail is intact"""
    import ctypes as C
    from pixie_amd import _lib
    lib = _lib.load()
    n, tail = 1025, 64
    p = torch.from_numpy(cloud("uniform1025")).to(hip_device)
    out = torch.full((n + tail,), float("nan"), dtype=torch.float32, device=hip_device)
    out[n:] = 12345.0
    need = lib.pixie_knn_mean_dist2_scratch_bytes(n)
    scratch = torch.empty((need,), dtype=torch.uint8, device=hip_device)
    rc = lib.pixie_knn_mean_dist2(C.c_void_p(p.data_ptr()), n, C.c_void_p(scratch.data_ptr()), need, C.c_void_p(out.data_ptr()), _lib.current_stream_ptr())
    _lib.check(rc, "pixie_knn_mean_dist2", lib=lib)
    got = out.cpu().numpy()
    assert np.all(got[n:] == 12345.0)
    assert np.array_equal(bits(got[:n]), bits(reference("uniform1025")))


def test_non_default_stream_and_non_contiguous_input(hip_device):
    from pixie_amd.simple_knn import distCUDA2
    p = cloud("uniform1023")
    wide = torch.zeros((len(p), 5), dtype=torch.float32, device=hip_device)
    wide[:, 1:4] = torch.from_numpy(p).to(hip_device)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    stream = torch.cuda.Stream(device=hip_device)
    stream.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(stream):
        got = distCUDA2(view)
    stream.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(reference("uniform1023")))


def test_argument_errors(hip_device):
    from pixie_amd.simple_knn import distCUDA2
    good = torch.zeros((8, 3), dtype=torch.float32, device=hip_device)
    with pytest.raises(ValueError, match="HIP device"):
        distCUDA2(good.cpu())
    with pytest.raises(ValueError, match="HIP device"):
        distCUDA2(np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        distCUDA2(torch.zeros((8, 4), dtype=torch.float32, device=hip_device))
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        distCUDA2(torch.zeros((24,), dtype=torch.float32, device=hip_device))
    with pytest.raises(ValueError, match="float32"):
        distCUDA2(good.double())
    assert distCUDA2(good[:0]).shape == (0,)
