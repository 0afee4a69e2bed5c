"""GPU operator tests of the conversion in the tile staging of conv3d_f16x3_body (stage_chunk): what a staged slot holds after the
prologue, the LayerNorm affine, the activation, the scale and the fp16 hi / lo split, and what a slot outside the input holds.

A slot outside the input loads element 0 of every channel plane (and of gamma / beta), runs the whole conversion and is replaced by
zero AFTER the activation.  The tests pin that behaviour; they do not tell one implementation of it from another:

  special values   +-0, fp32 subnormals and tiny normals among O(1) data through all six (prologue, activation) pipelines, with the
                   LayerNorm affine on and off; for SiLU the value entering the activation spans -110 .. +90, so the denominator
                   1 + exp(-t) reaches +inf (t below about -88.7: the quotient is -0)
  the mask         element 0 of every plane is NaN: only outputs whose receptive field holds voxel (0, 0, 0) may be non-finite
  exact padding    a tensor, and the same tensor inside a ring of explicit zeros, give equal bits where both are defined

Shapes are the small ones of tests/test_conv_staging_hip.py, so every tile has masked slots; n (items per thread and chunk) is
asserted from pixie_conv_tile_geometry as there.  They all run on the one-block-per-wave instantiations, which address a chunk's 16
channel planes with pointers; one case more, 16 x 64 x 128, is the smallest that runs on <3,2,2>, where the planes are addressed
through a buffer resource and a chunk with channels of both input tensors (24 | 24) takes a loop of its own.  Split-K is off.

Bounds: TOL and PER_TILE_TOL of tests/test_conv_variants_hip.py (2e-6 / 2e-6 for f16x3).  The reference alone, on the CPU, for these
inputs: the float64 result rounded to float32 is at rel-L2 2.49e-8 .. 2.57e-8 of itself over the whole tensor and at most 3.6e-8 on
the worst tile (test_the_reference_alone_is_far_inside_the_bounds asserts a quarter of each bound and prints the figures)."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import test_conv_staging_hip as tstage
import test_conv_variants_hip as tvar
from test_unet_hip import _amax_slots, _prologue_cpu, ref_conv, rel_l2

# the fields test_conv_staging_hip.geometry reads, under its names; sub (sub-pixel) is never set here
CC = namedtuple("CC", "id n cins cout dims k stride sub pro aff act")
CASES = [
    CC("4cubed-plain-none", 1, (16,), 64, (4, 4, 4), 3, 1, False, False, False, 0),
    CC("4cubed-pro-aff-leaky", 1, (16,), 64, (4, 4, 4), 3, 1, False, True, True, 1),
    CC("8cubed-plain-silu", 2, (16,), 64, (8, 8, 8), 3, 1, False, False, False, 2),
    CC("8cubed-24+24-pro-aff-silu", 2, (24, 24), 64, (8, 8, 8), 3, 1, False, True, True, 2),
    CC("odd-aff-leaky", 3, (16,), 32, (13, 9, 33), 3, 1, False, False, True, 1),
    CC("odd-pro-none", 3, (16,), 32, (13, 9, 33), 3, 1, False, True, False, 0),
    CC("odd-pro-silu", 3, (16,), 32, (13, 9, 33), 3, 1, False, True, False, 2),
    CC("stride2-24+24-pro-leaky", 6, (24, 24), 64, (9, 9, 33), 3, 2, False, True, False, 1),
    CC("stride2-plain-none", 6, (16,), 64, (9, 9, 33), 3, 2, False, False, False, 0),
    CC("pointwise-24+24-pro-aff-silu", 1, (24, 24), 64, (4, 8, 32), 1, 1, False, True, True, 2),
    # the smallest volume that gets 64 c_out and two voxel blocks per wave (<3,2,2>): those instantiations address the planes of a
    # chunk through a buffer resource, and a chunk with channels of both tensors (the second of the three here) through pointers
    CC("nb2-24+24-pro-aff-leaky", 4, (24, 24), 64, (16, 64, 128), 3, 1, False, True, True, 1),
]
NAN_CASES = [c for c in CASES if c.id in ("odd-aff-leaky", "odd-pro-silu", "stride2-24+24-pro-leaky", "pointwise-24+24-pro-aff-silu")]
SPECIAL = (0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30)
T_LO, T_HI = -110.0, 90.0      # SiLU: the span of the value entering the activation


def _operands(case, seed):
    g = torch.Generator().manual_seed(seed)
    dims, cin = tuple(case.dims), sum(case.cins)
    x = torch.cat([torch.randn((c,) + dims, generator=g) * (1.0 + 3.0 * i) for i, c in enumerate(case.cins)], 0)
    w = torch.randn((case.cout, cin) + (case.k,) * 3, generator=g) / np.sqrt(cin * case.k ** 3)
    b = torch.randn(case.cout, generator=g) + 0.5
    pro = (torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)) if case.pro else None
    affine = None
    if case.aff:      # |gamma| in 0.5 .. 1.5, so that a wanted activation input has a preimage of its own size
        sign = torch.where(torch.rand(dims, generator=g) < 0.5, -1.0, 1.0)
        affine = (sign * (torch.rand(dims, generator=g) + 0.5), torch.randn(dims, generator=g))
    return g, x, w, b, pro, affine


def _split(case, x):
    return list(torch.split(x, list(case.cins), 0))


@functools.lru_cache(maxsize=None)
def special_case(case):
    """host tensors and the float64 reference: randn with about 2 % of the elements replaced"""
    g, x, w, b, pro, affine = _operands(case, 8100 + CASES.index(case))
    hit = torch.rand(x.shape, generator=g) < 0.02
    n = int(hit.sum())
    vals = torch.tensor(SPECIAL, dtype=torch.float32)[torch.randint(len(SPECIAL), (n,), generator=g)]
    if case.act == 2:     # every second replaced element: the input whose activation argument is a point of T_LO .. T_HI
        t = torch.linspace(T_LO, T_HI, n, dtype=torch.float64)[torch.randperm(n, generator=g)]
        one, zero = torch.ones(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.float64)
        pa = pro[0].double()[:, None, None, None] * one if pro else one
        pb = pro[1].double()[:, None, None, None] * one if pro else zero
        gm = affine[0].double()[None] * one if affine else one
        bt = affine[1].double()[None] * one if affine else zero
        pre = (((t - bt[hit]) / gm[hit] - pb[hit]) / pa[hit]).float()
        vals = torch.where(torch.arange(n) % 2 == 0, pre, vals)
    x[hit] = vals
    parts = _split(case, x)
    ref = ref_conv(parts, w, b, case.stride, False, pro, affine, case.act, None)
    return parts, w, b, pro, affine, ref


def _run(ops, case, parts, w, b, pro, affine, in_bound=None, in_amax=None):
    dev = ops.device
    to = lambda t: t.to(dev) if t is not None else None
    dparts = [to(p) for p in parts]
    kw = dict(stride=case.stride, pro=tuple(map(to, pro)) if pro else None, affine=tuple(map(to, affine)) if affine else None,
              act=case.act, w16=ops.pack_conv16(to(w)))
    if in_bound is not None:
        kw["in_bound"] = in_bound
    else:
        kw["in_amax"] = in_amax if in_amax is not None else _amax_slots(ops, dparts)
    old = ops.split_k
    ops.split_k = False
    try:
        out = ops.conv(dparts, None, to(b), case.cout, case.k, **kw)
    finally:
        ops.split_k = old
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _errors(case, got, ref):
    geo, _ = tstage.geometry(case, "f16x3")
    return rel_l2(got, ref), tvar.per_tile_rel_l2(got, ref, geo["TZ"], geo["TY"], geo["TX"])


def test_the_cases_cover_what_selects_code_in_the_conversion():
    """(runs without a device: the geometry is a host function of the descriptor)"""
    for c in CASES:
        geo, _ = tstage.geometry(c, "f16x3")
        cs = tstage.staged_slots(c, geo)
        assert -(-cs // 256) == c.n and geo["slices"] == 1, (c.id, geo, cs)
    assert {(c.pro, c.act) for c in CASES} == {(p, a) for p in (False, True) for a in (0, 1, 2)}      # the six pipelines
    assert {c.aff for c in CASES} == {False, True} and any(c.aff and not c.pro for c in CASES)
    assert {min(c.n, 4) for c in CASES} == {1, 2, 3, 4}                                                # items per thread
    assert any(c.cins == (16,) for c in CASES)                                                          # one chunk
    straddling = [c for c in CASES if c.cins == (24, 24)]                                               # three, the split inside the second
    assert {c.k for c in straddling} == {1, 3} and {c.stride for c in straddling} == {1, 2} and any(c.n >= 4 for c in straddling)
    wide = [c for c in CASES if (lambda g: g["MB"] == 2 and g["NB"] >= 2)(tstage.geometry(c, "f16x3")[0])]
    assert any(c.k == 3 and c.cins == (24, 24) and c.pro and c.aff and c.act == 1 for c in wide)       # buffer-addressed planes, and the split
    assert any(c.dims == (4, 4, 4) for c in CASES) and any(c.dims == (8, 8, 8) for c in CASES) and any(c.dims == (13, 9, 33) for c in CASES)
    assert {(c.pro, c.act) for c in NAN_CASES} >= {(False, 1), (True, 1), (True, 2)} and {c.aff for c in NAN_CASES} == {False, True}
    assert any(c.k == 3 and c.stride == 1 and c.dims == (13, 9, 33) for c in NAN_CASES)
    assert any(c.stride == 2 for c in NAN_CASES) and any(c.k == 1 for c in NAN_CASES)


def test_the_reference_alone_is_far_inside_the_bounds():
    """(CPU) float64 reference rounded to float32 against itself, for the inputs with special values"""
    for c in CASES:
        ref = special_case(c)[5]
        whole, worst = _errors(c, ref.float().numpy(), ref.numpy())
        print(f"{c.id}: reference rounded to float32: rel-L2 whole {whole:.3e}, worst tile {worst:.3e}")
        assert whole < tvar.TOL["f16x3"] / 4 and worst < tvar.PER_TILE_TOL["f16x3"] / 4, (c.id, whole, worst)
        if c.act == 2:     # the inputs do what they were made for
            parts, _, _, pro, affine, _ = special_case(c)
            x = torch.cat(parts, 0)
            t = x * pro[0][:, None, None, None] + pro[1][:, None, None, None] if pro else x
            t = t * affine[0][None] + affine[1][None] if affine else t
            assert float(t.min()) < -100.0 and float(t.max()) > 85.0, (c.id, float(t.min()), float(t.max()))


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_special_values(ops, case):
    parts, w, b, pro, affine, ref = special_case(case)
    if pro is not None or affine is not None:     # a host bound, loose by 3x (the raw |x|max bounds nothing behind an affine)
        got = _run(ops, case, parts, w, b, pro, affine, in_bound=3.0 * float(_prologue_cpu(parts, pro, affine, case.act).abs().max()))
    else:
        got = _run(ops, case, parts, w, b, pro, affine)
    assert np.isfinite(got).all()
    whole, worst = _errors(case, got, ref.numpy())
    print(f"{case.id} n {case.n}: rel-L2 whole {whole:.3e}, worst tile {worst:.3e}")
    assert whole < tvar.TOL["f16x3"], whole
    assert worst < tvar.PER_TILE_TOL["f16x3"], worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", NAN_CASES, ids=[c.id for c in NAN_CASES])
def test_the_mask_is_a_select(ops, case):
    """Element 0 of every plane (and gamma[0], beta[0]) is NaN, which is what every slot outside the input loads."""
    _, x, w, b, pro, affine = _operands(case, 8200 + CASES.index(case))
    clean = x.clone()
    clean[:, 0, 0, 0] = 0.0
    x[:, 0, 0, 0] = float("nan")
    aff_clean = aff_nan = None
    if affine is not None:
        aff_clean, aff_nan = tuple(a.clone() for a in affine), tuple(a.clone() for a in affine)
        for a in aff_clean:
            a[0, 0, 0] = 0.0
        for a in aff_nan:
            a[0, 0, 0] = float("nan")
    ref = ref_conv(_split(case, clean), w, b, case.stride, False, pro, aff_clean, case.act, None).numpy()
    bound = 3.0 * float(_prologue_cpu(_split(case, clean), pro, aff_clean, case.act).abs().max())     # host bound: no amax pass sees the NaN
    got = _run(ops, case, _split(case, x), w, b, pro, aff_nan, in_bound=bound)
    pad = 1 if case.k == 3 else 0
    reach = pad // case.stride + 1        # outputs 0 .. reach - 1 of an axis read input 0
    sees = np.zeros(ref.shape, bool)
    sees[:, :reach, :reach, :reach] = True
    assert np.isfinite(got[~sees]).all(), f"{int((~np.isfinite(got[~sees])).sum())} non-finite outputs that cannot see voxel (0, 0, 0)"
    got = np.where(sees, ref, got)        # what may see the NaN is not compared
    whole, worst = _errors(case, got, ref)
    print(f"{case.id} n {case.n}: rel-L2 whole {whole:.3e}, worst tile {worst:.3e}")
    assert whole < tvar.TOL["f16x3"], whole
    assert worst < tvar.PER_TILE_TOL["f16x3"], worst


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1, 2])
def test_padding_is_an_exact_zero(ops, act):
    """act(0) = 0 without a prologue: a masked slot and a loaded zero stage the same bits, wherever the tile boundaries fall."""
    case = CC(f"ring-act{act}", 0, (16,), 32, (7, 6, 31), 3, 1, False, False, False, act)
    g = torch.Generator().manual_seed(8300 + act)
    t = torch.randn((16,) + case.dims, generator=g)
    w = torch.randn((case.cout, 16, 3, 3, 3), generator=g) / np.sqrt(16 * 27)
    b = torch.randn(case.cout, generator=g)
    ring = torch.zeros((16,) + tuple(d + 2 for d in case.dims))
    ring[:, 1:-1, 1:-1, 1:-1] = t
    amax = _amax_slots(ops, [t.to(ops.device)])     # the same scale for both launches
    alone = _run(ops, case, [t], w, b, None, None, in_amax=amax)
    inside = _run(ops, case._replace(dims=tuple(ring.shape[1:])), [ring], w, b, None, None, in_amax=amax)[:, 1:-1, 1:-1, 1:-1]
    assert alone.shape == inside.shape
    assert np.array_equal(alone[:, 1:-1, 1:-1, 1:-1], inside[:, 1:-1, 1:-1, 1:-1])     # receptive field inside t
    assert np.array_equal(alone, inside)                                               # and where the one is masked, the other loaded
