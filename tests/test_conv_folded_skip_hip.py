"""GPU tests of the folded 1x1x1 skip convolution (MyResBlock.skip_connection riding in the block's second 3^3 launch).

The skip has kernel instantiations of its own, conv3d_f16x3_skip_kernel<KS, MB, NB, STAGED>: register-fed (each lane loads the
B fragments of its own voxels, no LDS tile, no barrier) where every 16-channel chunk lies in one of the two skip tensors
(skip_c0 % 16 == 0), and staged through LDS where the parts meet inside a chunk (skip_c0 % 16 == 8).

Reference and bound: float64 torch on the CPU, main convolution plus 1x1x1 skip convolution, rel-L2 < 2e-6, and the epilogue
statistics against the written tensor with rtol 1e-5 (atol 1e-3 on the sum) -- the bounds of
tests/test_unet_hip.py::test_conv3d_folded_skip_convolution.  The two skip parts get different magnitudes (0.2 and 3), as there,
so a swapped part shows.

SMALL_CASES: the part splits x the volumes, with c_in, c_out and the four epilogue bodies (residual x statistics) cycling over
them; whole-tensor reference.  Volumes this small all plan <3,1,1> (no workspace: the tile shrinks), so COVERAGE_CASES add, for
every <KS, MB, NB> of the variant table and both skip forms, the smallest volume whose plan is that variant (64^3, 32 x 64 x 64,
16 x 64 x 64 voxels; c_out 64 / 32 for MB 2 / 1), asserted through ops.last_variant.  Their reference is taken on five z planes
(first, second, middle, last two) computed from the planes they read: the same reference, over the voxels where the tile
geometry changes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_unet_hip import _amax_slots, ref_conv, rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-6      # test_conv3d_folded_skip_convolution's


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    o = HipOps(hip_device)
    o.record_variant = True
    return o


PARTS = [(16,), (32,), (48,), (8, 24), (24, 8), (64, 64)]
VOLUMES = [(4, 4, 32), (3, 3, 5), (4, 4, 33), (5, 6, 97)]
COUTS = [64, 32, 128]
EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]     # (residual, statistics)

SMALL_CASES = []
for pi, parts in enumerate(PARTS):
    for vi, dims in enumerate(VOLUMES):
        n = pi * len(VOLUMES) + vi
        res, stats = EPILOGUES[(pi + vi) % 4]
        SMALL_CASES.append(pytest.param(parts, (16, 64)[(pi + vi) % 2], COUTS[(pi + 2 * vi) % 3], dims, res, stats, 100 + n,
                                        id=f"parts{'+'.join(map(str, parts))}-{'x'.join(map(str, dims))}"))


def make_inputs(cin, parts, cout, dims, k, res, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn((cin,) + dims, generator=g) + 0.5
    xs = [torch.randn((c,) + dims, generator=g) * (3.0 if i else 0.2) for i, c in enumerate(parts)]
    w = torch.randn((cout, cin) + (k,) * 3, generator=g) / np.sqrt(cin * k ** 3)
    b = torch.randn(cout, generator=g)
    ws = torch.randn((cout, sum(parts), 1, 1, 1), generator=g) / np.sqrt(sum(parts))
    bs = torch.randn(cout, generator=g)
    return h, xs, w, b, ws, bs, g


def launch(ops, h, xs, w, b, ws, bs, cout, k, residual, stats, out_size=None, skip_amax=None):
    """the folded launch, twice; returns (out, sums or None, amax slot)"""
    dev = ops.device
    dh, dxs = h.to(dev), [x.to(dev) for x in xs]
    fold = dict(parts=dxs, w16=ops.pack_conv16(ws.to(dev)), bias=bs.to(dev), amax=skip_amax if skip_amax is not None else _amax_slots(ops, dxs))
    kw = dict(w16=ops.pack_conv16(w.to(dev)), in_amax=_amax_slots(ops, [dh]), skip=fold, residual=residual.to(dev) if residual is not None else None)
    if out_size is not None:
        kw["out_size"] = out_size
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    if stats:
        out, sums = ops.conv([dh], None, b.to(dev), cout, k, out_amax=slot, **kw)
    else:
        out, sums = ops.conv([dh], None, b.to(dev), cout, k, **kw), None
    variant = ops.last_variant
    out2 = ops.conv([dh], None, b.to(dev), cout, k, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)       # fixed accumulation order, no atomics
    return out, sums, slot, variant


def check_stats(out, sums, slot, cout):
    o64 = out.double().reshape(cout, -1)
    assert torch.allclose(sums[:, 0], o64.sum(1), rtol=1e-5, atol=1e-3) and torch.allclose(sums[:, 1], (o64 * o64).sum(1), rtol=1e-5)
    assert abs(float(slot.view(torch.float32)) - float(out.abs().max())) < 1e-6 * float(out.abs().max())


def foldable_or_skip(ops, h, cout, k, xs):
    if not ops.skip_foldable(h, cout, k, xs):
        pytest.skip(f"the plan declines the fold for c_out {cout}, {k}^3 on {tuple(h.shape[1:])} (pixie_conv_skip_foldable)")


@pytest.mark.parametrize("parts,cin,cout,dims,res,stats,seed", SMALL_CASES)
def test_folded_skip_small(ops, parts, cin, cout, dims, res, stats, seed):
    h, xs, w, b, ws, bs, g = make_inputs(cin, parts, cout, dims, 3, res, seed)
    residual = torch.randn((cout,) + dims, generator=g) if res else None
    old = ops.split_k
    ops.split_k = False
    try:
        foldable_or_skip(ops, h, cout, 3, xs)
        out, sums, slot, variant = launch(ops, h, xs, w, b, ws, bs, cout, 3, residual, stats)
    finally:
        ops.split_k = old
    ref = ref_conv([h], w, b, residual=residual) + ref_conv(xs, ws, bs)
    err = rel_l2(out.cpu().numpy(), ref.numpy())
    print(f"folded skip parts {parts} c_in {cin} c_out {cout} {dims} res {res} stats {stats} variant {variant}: rel-L2 {err:.2e}")
    assert variant[1] == 1 and variant[0] // 100 == 3
    assert err < TOL, err
    if stats:
        check_stats(out, sums, slot, cout)


# (ksize, MB, NB) -> (c_out, dims): the smallest volume whose unsplit plan is that variant
COVERAGE_DIMS = {4: (64, 64, 64), 2: (32, 64, 64), 1: (16, 64, 64)}
COVERAGE_CASES = [pytest.param(k, mb, nb, parts, id=f"k{k}-mb{mb}-nb{nb}-{'staged' if parts[0] % 16 else 'registers'}")
                  for k in (3, 1) for mb in (2, 1) for nb in (4, 2, 1) for parts in ((16, 16), (8, 8))]


def ref_planes(h, xs, w, b, ws, bs, z0, z1):
    """float64 reference of output planes z0 .. z1 - 1, from the input planes they read"""
    D, p = h.shape[1], w.shape[-1] // 2
    lo, hi = max(z0 - p, 0), min(z1 + p, D)
    x = F.pad(h[:, lo:hi].double()[None], (0, 0, 0, 0, p - (z0 - lo), p - (hi - z1)))
    y = F.conv3d(x, w.double(), b.double(), padding=(0, p, p))[0]
    s = F.conv3d(torch.cat(xs, 0)[:, z0:z1].double()[None], ws.double(), bs.double())[0]
    return y + s


@pytest.mark.parametrize("k,mb,nb,parts", COVERAGE_CASES)
def test_folded_skip_every_instantiation(ops, k, mb, nb, parts):
    cout, dims, cin = (64 if mb == 2 else 32), COVERAGE_DIMS[nb], 16
    h, xs, w, b, ws, bs, g = make_inputs(cin, parts, cout, dims, k, False, 7000 + 100 * k + 10 * mb + nb + parts[0])
    old = ops.split_k
    ops.split_k = False
    try:
        foldable_or_skip(ops, h, cout, k, xs)
        out, sums, slot, variant = launch(ops, h, xs, w, b, ws, bs, cout, k, None, True)
    finally:
        ops.split_k = old
    assert variant == (k * 100 + mb * 10 + nb, 1), variant
    D = dims[0]
    o = out.cpu()
    worst = 0.0
    for z0, z1 in ((0, 2), (D // 2, D // 2 + 1), (D - 2, D)):
        err = rel_l2(o[:, z0:z1].numpy(), ref_planes(h, xs, w, b, ws, bs, z0, z1).numpy())
        worst = max(worst, err)
        assert err < TOL, (z0, z1, err)
    print(f"folded skip <{k},{mb},{nb}> parts {parts} c_out {cout} {dims}: worst plane group rel-L2 {worst:.2e}")
    check_stats(out, sums, slot, cout)


@pytest.mark.parametrize("parts", [(16, 16), (8, 24)], ids=["registers", "staged"])
def test_folded_skip_masked_lanes_do_not_leak(ops, parts):
    """Ragged tiles under an odd-grid crop: the skip tensors hold 1e30 at voxels behind the cropped output range (y = 6 and
    x = 97 of a 5 x 7 x 98 input cropped to 5 x 6 x 97).  No output voxel reads them, and the lanes of the ragged tiles that have
    no output voxel are masked: a leak shows as inf / NaN or a huge error.  The skip's |x|max slots are those of the region that
    is read (a valid bound for every value the launch uses): with 1e30 in the bound, the scale would flush the skip to zero."""
    cin, cout, dims, crop = 16, 64, (5, 7, 98), (5, 6, 97)
    h, xs, w, b, ws, bs, g = make_inputs(cin, parts, cout, dims, 3, False, 4242 + parts[0])
    amax = _amax_slots(ops, [x[:, :crop[0], :crop[1], :crop[2]].contiguous().to(ops.device) for x in xs])
    for x in xs:
        x[:, :, crop[1]:, :] = 1e30
        x[:, :, :, crop[2]:] = 1e30
    old = ops.split_k
    ops.split_k = False
    try:
        foldable_or_skip(ops, h, cout, 3, xs)
        out, sums, slot, variant = launch(ops, h, xs, w, b, ws, bs, cout, 3, None, True, out_size=crop, skip_amax=amax)
    finally:
        ops.split_k = old
    assert tuple(out.shape) == (cout,) + crop and bool(torch.isfinite(out).all())
    ref = (ref_conv([h], w, b) + ref_conv(xs, ws, bs))[:, :crop[0], :crop[1], :crop[2]]
    err = rel_l2(out.cpu().numpy(), ref.numpy())
    print(f"folded skip, 1e30 behind the crop, parts {parts}, variant {variant}: rel-L2 {err:.2e}")
    assert err < TOL, err
    check_stats(out, sums, slot, cout)
