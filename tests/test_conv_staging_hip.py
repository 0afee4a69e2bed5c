"""GPU operator tests of the tile staging of conv3d_f16x3_body (stage_chunk): one HipOps.conv launch per case against a float64
torch convolution on the CPU.

Per 16-channel chunk a thread owns the items k = 0 .. n - 1 at the halo slots tid + 256 k, n = ceil(CS / 256), CS = HX HY HZ of the
tile, and walks them as a rotating two-set pipeline: a loop over pairs of items, then a peeled tail of two items (n even) or one
(n odd); the last item is ragged wherever CS is no multiple of 256.  What selects code there is n, the (prologue, activation)
pair (six straight-line pipelines), the LayerNorm affine (its loads are issued either way, its values used or replaced), the
chunk count and where the two-part input splits.  The cases cross those; n is asserted for each from pixie_conv_tile_geometry:

  n = 1   4^3, 3^3: CS = 216 < 256, 40 threads own no item; and a 1x1x1 convolution at NB 1: CS = 128
  n = 2   8^3 (10 x 6 x 6 = 360); the sub-pixel up-convolution (34 x 5 x 3 = 510)
  n = 3   13 x 9 x 33 (34 x 6 x 3 = 612): one pair and a single item; ragged border tiles on all three axes
  n = 4   16 x 64 x 128 at NB 2 (34 x 6 x 4 = 816): one pair and a tail of two
  n = 5   32 x 64 x 128, the dominant tile (34 x 6 x 6 = 1224), with the dominant pipeline (prologue, LayerNorm affine, LeakyReLU)
  n = 6   stride 2 from 9 x 9 x 33 (33 x 9 x 5 = 1485): two pairs and a tail of two

Across them: c_in 16 (one chunk) and c_in 48 = 24 | 24 (three chunks, the split inside the second); prologue on / off with each of
activation 0 / 1 / 2; LayerNorm affine on / off, once without a prologue; odd extents 9 and 13; KS = 1; all-negative inputs
through LeakyReLU.  The exact-fp32 body keeps the two-items-per-pass loop; the small cases run on it too.

Bounds: the whole-tensor and per-tile rel-L2 bounds of tests/test_conv_variants_hip.py for the same precision (imported).  The
reference alone, on the CPU, for these seeds: the float64 result rounded to float32 is at rel-L2 2.5e-8 .. 2.7e-8 of itself over
the whole tensor and at most 3.2e-8 on the worst tile (bounds 2e-6 / 1e-5)."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import test_conv_variants_hip as tvar
from _conv_census import operator_desc, tile_geometry
from test_unet_hip import _amax_slots, _prologue_cpu, ref_conv, rel_l2

# pro: per-channel scale/shift; aff: per-voxel LayerNorm gamma/beta; act 0 none, 1 LeakyReLU, 2 SiLU; neg: every input below zero
SC = namedtuple("SC", "id n cins cout dims k stride sub pro aff act neg f32")
CASES = [
    SC("n1-4cubed", 1, (16,), 64, (4, 4, 4), 3, 1, False, False, False, 0, False, True),
    SC("n1-pointwise", 1, (24, 24), 64, (4, 8, 32), 1, 1, False, True, True, 2, False, True),
    SC("n2-8cubed", 2, (24, 24), 64, (8, 8, 8), 3, 1, False, True, False, 0, False, True),
    SC("n2-subpixel", 2, (16,), 64, (8, 16, 32), 3, 1, True, True, False, 2, False, False),
    SC("n3-odd", 3, (16,), 32, (13, 9, 33), 3, 1, False, False, True, 2, False, True),
    SC("n4-nb2", 4, (16,), 64, (16, 64, 128), 3, 1, False, False, False, 1, True, False),
    SC("n5-dominant", 5, (16,), 64, (32, 64, 128), 3, 1, False, True, True, 1, False, False),
    SC("n6-stride2", 6, (24, 24), 64, (9, 9, 33), 3, 2, False, True, False, 1, False, True),
]


def staged_slots(case, geo):
    """CS = HX HY HZ of the tile the library reports: the halo'd extent a workgroup stages per chunk.  pixie_conv_tile_geometry
    reports TX, TY, TZ and not the halo extents, so the halo formula of the launch plan (conv_plan.h, where conv_plan() sets
    p.HX / p.HY / p.HZ) is restated here: the asserted n checks the cases against that formula, not the formula itself."""
    if case.sub:      # the tile lies over the stored voxels; one voxel of halo on the side the parity reads, x on both
        return (geo["TX"] + 2) * (geo["TY"] + 1) * (geo["TZ"] + 1)
    return int(np.prod([(geo[t] - 1) * case.stride + case.k for t in ("TX", "TY", "TZ")]))


def geometry(case, prec):
    desc, oshape = operator_desc(prec, case.cins, case.cout, case.dims, case.k, stride=case.stride, upsample=case.sub,
                                 subpixel=case.sub and prec == "f16x3",
                                 prologue="channel+spatial" if (case.pro and case.aff) else ("channel" if case.pro else "none"),
                                 split_k=False)
    return tile_geometry(desc), oshape


@functools.lru_cache(maxsize=None)
def make_case(case):
    """host tensors of a case and its float64 reference, shared by the two precisions"""
    g = torch.Generator().manual_seed(7000 + CASES.index(case))
    dims = tuple(case.dims)
    cin = sum(case.cins)
    if case.neg:
        parts = [-(torch.randn((c,) + dims, generator=g).abs() * (1.0 + 3.0 * i) + 0.5) for i, c in enumerate(case.cins)]
    else:
        parts = [torch.randn((c,) + dims, generator=g) * (1.0 + 3.0 * i) for i, c in enumerate(case.cins)]
        parts[0] += 3.0
    w = torch.randn((case.cout, cin) + (case.k,) * 3, generator=g) / np.sqrt(cin * case.k ** 3)
    b = torch.randn(case.cout, generator=g) + 0.5
    pro = (torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)) if case.pro else None
    affine = (torch.randn(dims, generator=g), torch.randn(dims, generator=g)) if case.aff else None
    ref = ref_conv(parts, w, b, case.stride, case.sub, pro, affine, case.act, None)
    return parts, w, b, pro, affine, ref


def test_the_cases_cover_what_selects_code_in_the_staging():
    """(runs without a device: the geometry is a host function of the descriptor)"""
    assert {c.n for c in CASES} >= {1, 2, 3, 4, 5} and any(c.n >= 6 and c.stride == 2 for c in CASES)
    for c in CASES:
        geo, _ = geometry(c, "f16x3")
        cs = staged_slots(c, geo)
        assert -(-cs // 256) == c.n and geo["slices"] == 1, (c.id, geo, cs)
    assert any(staged_slots(c, geometry(c, "f16x3")[0]) < 256 for c in CASES)                   # threads without an item
    assert {(c.pro, c.act) for c in CASES} == {(p, a) for p in (False, True) for a in (0, 1, 2)}
    assert {c.aff for c in CASES} == {False, True} and any(c.aff and not c.pro for c in CASES)
    assert any(c.cins == (16,) for c in CASES) and any(c.cins == (24, 24) for c in CASES)       # one chunk; three, split inside one
    assert any(9 in c.dims and 13 in c.dims for c in CASES)
    assert any(c.k == 1 for c in CASES) and any(c.sub for c in CASES) and any(c.neg and c.act == 1 for c in CASES)
    dom = next(c for c in CASES if c.n == 5)
    geo, _ = geometry(dom, "f16x3")
    assert (geo["TX"], geo["TY"], geo["TZ"], geo["MB"], geo["NB"]) == (32, 4, 4, 2, 4) and dom.pro and dom.aff and dom.act == 1


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


PARAMS = [pytest.param(c, p, id=f"{c.id}-{p}") for c in CASES for p in (("f16x3", "f32") if c.f32 else ("f16x3",))]


@pytest.mark.gpu
@pytest.mark.parametrize("case,prec", PARAMS)
def test_staging(ops, case, prec):
    geo, oshape = geometry(case, prec)
    sub = case.sub and prec == "f16x3"
    if prec == "f16x3":
        assert -(-staged_slots(case, geo) // 256) == case.n, geo
    parts, w, b, pro, affine, ref = make_case(case)
    assert tuple(oshape) == tuple(ref.shape)
    dev = ops.device
    to = lambda t: t.to(dev) if t is not None else None
    dparts = [to(p) for p in parts]
    kw = dict(stride=case.stride, upsample=case.sub, pro=tuple(map(to, pro)) if pro else None,
              affine=tuple(map(to, affine)) if affine else None, act=case.act)
    old = ops.split_k
    ops.split_k = False
    try:
        if prec == "f32":
            out = ops.conv(dparts, ops.pack_conv(to(w)), to(b), case.cout, case.k, **kw)
        else:
            kw.update(w16=ops.pack_conv_subpixel(to(w)) if sub else ops.pack_conv16(to(w)), subpixel=sub)
            if pro is not None or affine is not None:     # the raw |x|max bounds nothing behind an affine: a host bound, loose by 3x
                kw["in_bound"] = 3.0 * float(_prologue_cpu(parts, pro, affine, case.act).abs().max())
            else:
                kw["in_amax"] = _amax_slots(ops, dparts)
            out = ops.conv(dparts, None, to(b), case.cout, case.k, **kw)
    finally:
        ops.split_k = old
    torch.cuda.synchronize()
    o, refn = out.cpu().numpy(), ref.numpy()
    m = 2 if sub else 1
    whole, worst = rel_l2(o, refn), tvar.per_tile_rel_l2(o, refn, m * geo["TZ"], m * geo["TY"], m * geo["TX"])
    print(f"{case.id} {prec} n {case.n} tile {geo['TZ']}x{geo['TY']}x{geo['TX']}: rel-L2 whole {whole:.3e}, worst tile {worst:.3e}")
    assert whole < tvar.TOL[prec], whole
    assert worst < tvar.PER_TILE_TOL[prec], worst
