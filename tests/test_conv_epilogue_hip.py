"""GPU operator tests of the interior-tile ("full") epilogue of conv3d_f16x3_body: one HipOps.conv launch per case against a float64
torch convolution on the CPU.

The epilogue dispatches once on (residual, statistics) into four straight-line bodies, adds the bias (+ folded-skip bias; a missing
one is a null pointer) on the way into the LDS transpose, and fetches the residual a group of rows ahead of the stores.  The cases
cross what selects code there:

* c_in 16 (one chunk), c_out 64 -> MB 2 and c_out 32 -> MB 1; the voxel count picks NB 4, 2 and 1 in turn (asserted from
  pixie_conv_tile_geometry); every tile full, two or more tiles per axis;
* bias only, bias + folded-skip bias (f16x3), no bias;
* residual on / off crossed with statistics on / off on the f16x3 path; the exact-fp32 path has no epilogue statistics
  (HipOps.conv takes out_amax on the f16x3 path only), so it runs residual on / off;
* one launch whose last x tile is ragged while OW % 4 = 0: full-path and fallback workgroups side by side;
* one sub-pixel up-convolution with residual and statistics.

The c_out 32 cases use the first 32 filters of the c_out 64 weights, so three float64 convolutions serve all rows.  Bounds: the
whole-tensor rel-L2 bound of tests/test_conv_variants_hip.py for the same precision (imported); statistics as
test_unet_hip.test_conv3d_epilogue_statistics: finalised sums against float64 sums of the RETURNED output rel-L2 < 1e-6, |x|max
bit-equal.  The reference alone, on the CPU, for these seeds: the float64 result rounded to float32 is at rel-L2 2.5e-8 of itself
(bounds 2e-6 / 1e-5), and float32 sums over the launch's tiles added up in float64 -- what the epilogue and its finalise do -- are at
rel-L2 1.8e-9 .. 2.6e-9 of the float64 sums of the same tensor (bound 1e-6)."""
import functools

import numpy as np
import pytest
import torch

import test_conv_variants_hip as tvar
from _conv_census import operator_desc, tile_geometry
from test_unet_hip import _amax_slots, ref_conv, rel_l2

pytestmark = pytest.mark.gpu

CIN = 16
DIMS = {4: (32, 64, 128), 2: (16, 64, 128), 1: (8, 64, 128)}      # NB -> the smallest full-tile extents that select it
RAGGED = (8, 64, 144)        # x tiles of 32: four full, one of 16; 144 % 4 = 0
SUB = (8, 16, 32)            # stored extents of the sub-pixel case: output 16 x 32 x 64


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


@functools.lru_cache(maxsize=None)
def base(dims, up=False):
    """inputs, 64 filters and the float64 convolution without bias, shared by every case on these extents"""
    g = torch.Generator().manual_seed(4000 + sum(dims))
    x = torch.randn((CIN,) + dims, generator=g) + 3.0
    w = torch.randn((64, CIN, 3, 3, 3), generator=g) / np.sqrt(CIN * 27)
    b = torch.randn(64, generator=g) + 0.5
    ref = ref_conv([x], w, torch.zeros(64), 1, up, None, None, 0, None)
    res = torch.randn(ref.shape, generator=g)
    xs = torch.randn((CIN,) + dims, generator=g)
    ws = torch.randn((64, CIN, 1, 1, 1), generator=g) / np.sqrt(CIN)
    bs = torch.randn(64, generator=g)
    return x, w, b, ref, res, (xs, ws, bs)


@functools.lru_cache(maxsize=None)
def skip_ref(dims):
    xs, ws, bs = base(dims)[5]
    return ref_conv([xs], ws, bs)


def run_case(ops, prec, dims, cout, bias, residual, stats, *, sub=False):
    x, w, b, ref, res, (xs, ws, bs) = base(dims, sub)
    dev = ops.device
    w, b, ref, res = w[:cout], b[:cout], ref[:cout], res[:cout]
    expect = ref.clone()
    kw = dict(upsample=sub)
    dx = x.to(dev)
    if bias != "none":
        expect += b.double()[:, None, None, None]
    if bias == "bias+skip":
        expect += skip_ref(dims)[:cout]
    if residual:
        expect += res.double()
        kw["residual"] = res.to(dev)
    old = ops.split_k
    ops.split_k = False
    try:
        if prec == "f32":
            out = ops.conv([dx], ops.pack_conv(w.to(dev)), b.to(dev) if bias != "none" else None, cout, 3, **kw)
            sums = slot = None
        else:
            kw.update(w16=ops.pack_conv_subpixel(w.to(dev)) if sub else ops.pack_conv16(w.to(dev)), subpixel=sub, in_amax=_amax_slots(ops, [dx]))
            if bias == "bias+skip":
                dxs = [xs.to(dev)]
                kw["skip"] = dict(parts=dxs, w16=ops.pack_conv16(ws[:cout].to(dev)), bias=bs[:cout].to(dev), amax=_amax_slots(ops, dxs))
            slot = torch.zeros(1, dtype=torch.int32, device=dev) if stats else None
            got = ops.conv([dx], None, b.to(dev) if bias != "none" else None, cout, 3, out_amax=slot, **kw)
            out, sums = got if stats else (got, None)
    finally:
        ops.split_k = old
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(expect.shape)
    o = out.cpu()
    err = rel_l2(o.numpy(), expect.numpy())
    print(f"{prec} {dims} c_out {cout} bias {bias} residual {int(residual)} stats {int(stats)}: rel-L2 {err:.3e}")
    assert err < tvar.TOL[prec], err
    if stats:
        assert sums is not None and tuple(sums.shape) == (cout, 2)
        o64 = o.double().reshape(cout, -1)
        want = torch.stack([o64.sum(1), (o64 * o64).sum(1)], 1)
        es = rel_l2(sums.cpu().numpy(), want.numpy())
        print(f"    finalised sums against float64 sums of the output: rel-L2 {es:.3e}")
        assert es < 1e-6, es
        assert float(slot.view(torch.float32).item()) == float(o.abs().max())


def geometry(prec, dims, cout, *, residual=False, stats=False, skip=False, sub=False):
    desc, _ = operator_desc(prec, (CIN,), cout, dims, 3, upsample=sub, subpixel=sub, residual=residual, stats=stats,
                            skip_cins=(CIN,) if skip else None, split_k=False)
    return tile_geometry(desc)


BIAS = ["bias", "bias+skip", "none"]
FULL_CASES = []
for _nb in (4, 2, 1):
    for _cout in (64, 32):
        for _i, (_res, _stats) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
            # every bias form on the flagship class <3,2,4>; one per body, in rotation, on the others
            for _bias in (BIAS if (_nb, _cout) == (4, 64) else [BIAS[(_i + _nb + _cout // 32) % 3]]):
                FULL_CASES.append(pytest.param("f16x3", _nb, _cout, _bias, _res, _stats,
                                               id=f"f16x3-nb{_nb}-c{_cout}-{_bias}-res{int(_res)}-stats{int(_stats)}"))
        for _res in (False, True):
            _bias = "bias" if (_res + _nb) % 2 else "none"
            FULL_CASES.append(pytest.param("f32", _nb, _cout, _bias, _res, False, id=f"f32-nb{_nb}-c{_cout}-{_bias}-res{int(_res)}"))


@pytest.mark.parametrize("prec,nb,cout,bias,residual,stats", FULL_CASES)
def test_full_tile_epilogue(ops, prec, nb, cout, bias, residual, stats):
    dims = DIMS[nb]
    geo = geometry(prec, dims, cout, residual=residual, stats=stats, skip=bias == "bias+skip")
    assert geo["NB"] == nb and geo["MB"] == cout // 32 and geo["slices"] == 1 and geo["epi_lds"], geo
    assert all(d % t == 0 and d // t >= 2 for d, t in zip(dims, (geo["TZ"], geo["TY"], geo["TX"]))), geo      # all tiles full, >= 2 per axis
    run_case(ops, prec, dims, cout, bias, residual, stats)


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_full_and_ragged_tiles_in_one_launch(ops, prec):
    stats = prec == "f16x3"
    geo = geometry(prec, RAGGED, 64, residual=True, stats=stats)
    assert geo["epi_lds"] and geo["slices"] == 1 and RAGGED[2] % 4 == 0 and RAGGED[2] % geo["TX"] != 0 and geo["tiles_x"] >= 2, geo
    run_case(ops, prec, RAGGED, 64, "bias", True, stats)


def test_subpixel_full_tiles(ops):
    geo = geometry("f16x3", SUB, 64, residual=True, stats=True, sub=True)
    assert geo["epi_lds"] and geo["slices"] == 1 and all(d % t == 0 for d, t in zip(SUB, (geo["TZ"], geo["TY"], geo["TX"]))), geo
    run_case(ops, "f16x3", SUB, 64, "bias", True, True, sub=True)
