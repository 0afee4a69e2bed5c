"""GPU tests of the statistics a split-K launch takes in its reduce, and of the merged finalise (pixie_stats_norm_finalize).

A split-K layer's slices are added by a reduce kernel.  Asked for statistics (pixie_conv_desc.d_out_stats, HipOps.conv with
defer_stats), that kernel also leaves per channel and segment the sum and the sum of squares of the values it stores, in
float64, and the tensor's |x|max; pixie_stats_finalize / pixie_stats_norm_finalize add the segments up.  Checked here:

* sums, sums of squares and |x|max against float64 sums of the RETURNED tensor, relative error per channel < 1e-5 (the bound of
  the epilogue-statistics tests; the reduce adds in float64 throughout, so it has a wide margin), |x|max bit-equal;
* the output is bit-equal to the reduce without statistics (same slice order, then bias, then residual), and two launches
  agree bit for bit in the output and in the sums;
* the merged finalise against the two-launch route (pixie_stats_finalize + pixie_norm_finalize) and against float64.

Bias sign rule (tests/test_conv_variants_hip.py): the bias of a channel, magnitude 1 + |N(0,1)|, has the sign of that channel's
mean output, so that no channel's sum cancels and the relative error of a sum speaks about the summation.  The sign is taken
from a launch with zero bias; it only conditions the data and is no reference.

Tolerance of the affine (a, b), from float64 reference values only.  With m = mean, q = mean of squares, v = q - m^2 of the
float64 reference and e = 1e-5 the relative bound on the two sums: |dm| <= e |m|, |dv| <= e (q + 2 m^2), a = (v + eps)^-1/2 so
|da| <= a |dv| / (2 (v + eps)), and b = -m a (times the weight, plus the bias) so |db| <= |w| (|m| |da| + a |dm|); one float32
rounding (2^-23 relative) is added to each."""
import numpy as np
import pytest
import torch

from test_conv_subpixel_hip import SUBPIXEL_SPLIT_K_SHAPES
from test_unet_hip import SPLIT_K_SHAPES, _amax_slots

pytestmark = pytest.mark.gpu

STAT_TOL = 1e-5


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


# (cin parts, cout, dims, ksize, sub-pixel up-conv, residual)
REDUCE_CASES = (
    [pytest.param((cins, cout, dims, k, False, False), id=f"k{k}-{'+'.join(map(str, cins))}to{cout}-{'x'.join(map(str, dims))}")
     for cins, cout, dims, k in SPLIT_K_SHAPES]
    + [pytest.param((cins, cout, dims, 3, True, False), id=f"sub-{'+'.join(map(str, cins))}to{cout}-{'x'.join(map(str, dims))}")
       for cins, cout, dims in SUBPIXEL_SPLIT_K_SHAPES]
    + [pytest.param(((128,), 128, (32, 32, 32), 3, False, True), id="res-128to128-32x32x32"),
       pytest.param(((256,), 256, (16, 16, 16), 3, False, True), id="res-256to256-16x16x16"),
       pytest.param(((256,), 256, (5, 5, 5), 3, False, True), id="res-256to256-5x5x5")])     # odd extent: the scalar form of the reduce


def _launch(ops, case, seed):
    """-> (conv(bias) -> (out, PendingStats, slot), conv without statistics, c_out)"""
    from pixie_amd.unet import PendingStats
    cins, cout, dims, k, sub, with_res = case
    g = torch.Generator().manual_seed(seed)
    dev = ops.device
    parts = [(torch.randn((c,) + dims, generator=g) * (4.0 if i else 1.0)).to(dev) for i, c in enumerate(cins)]
    cin = sum(cins)
    w = (torch.randn((cout, cin, k, k, k), generator=g) / np.sqrt(cin * k ** 3)).to(dev)
    bmag = 1.0 + torch.randn(cout, generator=g).abs()
    odims = tuple(2 * d for d in dims) if sub else dims
    res = torch.randn((cout,) + odims, generator=g).to(dev) if with_res else None
    kw = dict(w16=ops.pack_conv_subpixel(w) if sub else ops.pack_conv16(w), in_amax=_amax_slots(ops, parts), residual=res)
    if sub:
        kw.update(upsample=True, subpixel=True)
    zero = ops.conv(parts, None, torch.zeros(cout, device=dev), cout, k, **kw)
    mean = zero.double().reshape(cout, -1).mean(1).cpu()
    b = torch.where(mean < 0, -bmag, bmag).to(dev)          # the bias sign rule

    def with_stats():
        slot = torch.zeros(1, dtype=torch.int32, device=dev)
        out, pend = ops.conv(parts, None, b, cout, k, out_amax=slot, defer_stats=True, **kw)
        assert isinstance(pend, PendingStats), "this shape must split and take its statistics in the reduce"
        assert pend.desc.d_workspace, "this shape must split"
        return out, pend, slot

    return with_stats, (lambda: ops.conv(parts, None, b, cout, k, **kw)), cout


def _rel(got, ref):
    return float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", REDUCE_CASES)
def test_splitk_reduce_statistics(ops, case):
    with_stats, plain, cout = _launch(ops, case, 211)
    out, pend, slot = with_stats()
    sums = ops.stats_finalize(pend)
    out2, pend2, slot2 = with_stats()
    sums2 = ops.stats_finalize(pend2)
    parent = plain()                                      # the reduce without statistics: splitk_reduce_kernel
    torch.cuda.synchronize()
    o64 = out.double().reshape(cout, -1)
    s = sums.cpu()
    e1, e2 = _rel(s[:, 0], o64.sum(1).cpu()), _rel(s[:, 1], (o64 * o64).sum(1).cpu())
    print(f"reduce statistics against float64 of the returned tensor: sum {e1:.2e}, sum of squares {e2:.2e} (worst channel, relative)")
    assert tuple(s.shape) == (cout, 2)
    assert e1 < STAT_TOL and e2 < STAT_TOL, (e1, e2)
    assert float(slot.view(torch.float32).item()) == float(out.abs().max())      # |x|max, same float bits
    assert torch.equal(out, parent)                       # same slice order, same bias and residual order
    assert torch.equal(out, out2) and torch.equal(sums, sums2) and int(slot.item()) == int(slot2.item())


def _affine_ref(o64_parts, mode, groups, weight, bias, eps=1e-5):
    """float64 (a, b, tol_a, tol_b) of the prologue affine over the channel concatenation of the given (c, spatial) tensors"""
    x = torch.cat(o64_parts, 0)
    c = x.shape[0]
    m, q = x.mean(1), (x * x).mean(1)
    if mode == 1:
        cpg = c // groups
        m = m.reshape(groups, cpg).mean(1).repeat_interleave(cpg)
        q = q.reshape(groups, cpg).mean(1).repeat_interleave(cpg)
    v = (q - m * m).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(v + eps)
    w = weight.double() if (mode == 1 and weight is not None) else torch.ones(c, dtype=torch.float64)
    bb = bias.double() if (mode == 1 and bias is not None) else torch.zeros(c, dtype=torch.float64)
    a, b = rstd * w, bb - m * rstd * w
    dm, dv = STAT_TOL * m.abs(), STAT_TOL * (q + 2 * m * m)
    da = rstd * dv / (2 * (v + eps))
    f32 = 2.0 ** -23
    tol_a = w.abs() * da + f32 * a.abs()
    tol_b = w.abs() * (m.abs() * da + rstd * dm) + f32 * (b.abs() + bb.abs())
    return a, b, tol_a, tol_b


# the producer of each part: a split-K launch (float64 segment partials); test_merged_finalise_of_tile_partials has the unsplit one
SPLIT = ((256,), 256, (16, 16, 16), 3, False, True)
FINALISE_CASES = [
    pytest.param((SPLIT,), 0, 1, id="layernorm-split"),
    pytest.param((SPLIT,), 1, 32, id="groupnorm32-split"),
    pytest.param((SPLIT, SPLIT), 0, 1, id="layernorm-cat-both-pending"),
    pytest.param((SPLIT, None), 0, 1, id="layernorm-cat-second-final"),
    pytest.param((None, SPLIT), 1, 32, id="groupnorm32-cat-first-final"),
]


@pytest.mark.parametrize("producers,mode,groups", FINALISE_CASES)
def test_merged_finalise(ops, producers, mode, groups):
    """One launch from the producers' partials to (sums, a, b) against the two-launch route and float64.  `None` in producers:
    that part's sums are final already (taken by pixie_stats_finalize beforehand)."""
    dev = ops.device
    outs, ents, old_sums = [], [], []
    for i, prod in enumerate(producers):
        with_stats, _, cout = _launch(ops, prod if prod is not None else SPLIT, 307 + i)
        out, pend, _ = with_stats()
        final = ops.stats_finalize(pend)
        outs.append(out); old_sums.append(final)
        ents.append(pend if prod is not None else final.clone())
    c = sum(o.shape[0] for o in outs)
    spatial = outs[0][0].numel()
    g = torch.Generator().manual_seed(5)
    weight = (1 + 0.3 * torch.randn(c, generator=g)) if mode == 1 else None
    bias = torch.randn(c, generator=g) if mode == 1 else None
    to = lambda t: t.to(dev) if t is not None else None
    a_old, b_old = ops.norm_finalize(torch.cat(old_sums, 0), spatial, mode, groups=groups, weight=to(weight), bias=to(bias))
    a, b, sums = ops.stats_norm_finalize(ents, spatial, mode, groups=groups, weight=to(weight), bias=to(bias))
    torch.cuda.synchronize()
    a_ref, b_ref, tol_a, tol_b = _affine_ref([o.double().reshape(o.shape[0], -1).cpu() for o in outs], mode, groups, weight, bias)
    for o, sm in zip(outs, sums):
        o64 = o.double().reshape(o.shape[0], -1)
        e1, e2 = _rel(sm[:, 0].cpu(), o64.sum(1).cpu()), _rel(sm[:, 1].cpu(), (o64 * o64).sum(1).cpu())
        print(f"merged finalise sums against float64: sum {e1:.2e}, sum of squares {e2:.2e}")
        assert e1 < STAT_TOL and e2 < STAT_TOL, (e1, e2)
    ea, eb = (a.cpu().double() - a_ref).abs(), (b.cpu().double() - b_ref).abs()
    eoa, eob = (a_old.cpu().double() - a_ref).abs(), (b_old.cpu().double() - b_ref).abs()
    print(f"affine against float64, worst |err| / tolerance: merged a {float((ea / tol_a).max()):.2e} b {float((eb / tol_b).max()):.2e}; "
          f"two launches a {float((eoa / tol_a).max()):.2e} b {float((eob / tol_b).max()):.2e}; "
          f"merged == two launches bit for bit: {torch.equal(a, a_old) and torch.equal(b, b_old)}")
    assert bool((ea <= tol_a).all()) and bool((eb <= tol_b).all())
    assert bool((eoa <= tol_a).all()) and bool((eob <= tol_b).all())
    # against the old route itself: both lie within the tolerance of the same reference
    assert bool(((a.cpu().double() - a_old.cpu().double()).abs() <= 2 * tol_a).all())
    assert bool(((b.cpu().double() - b_old.cpu().double()).abs() <= 2 * tol_b).all())


def test_merged_finalise_of_tile_partials(ops):
    """The same launch over the float32 per-tile partials of an UNSPLIT conv epilogue (the 64^3 / 128^3 layers)."""
    from pixie_amd.unet import PendingStats
    dev = ops.device
    g = torch.Generator().manual_seed(401)
    cin, cout, dims = 64, 64, (32, 32, 32)
    x = torch.randn((cin,) + dims, generator=g).to(dev)
    w = (torch.randn((cout, cin, 3, 3, 3), generator=g) / np.sqrt(cin * 27)).to(dev)
    bmag = 1.0 + torch.randn(cout, generator=g).abs()
    kw = dict(w16=ops.pack_conv16(w), in_amax=_amax_slots(ops, [x]))
    zero = ops.conv([x], None, torch.zeros(cout, device=dev), cout, 3, **kw)
    mean = zero.double().reshape(cout, -1).mean(1).cpu()
    b = torch.where(mean < 0, -bmag, bmag).to(dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.split_k = False          # as test_conv3d_epilogue_statistics does: at this size the layer would split otherwise
    try:
        out, pend = ops.conv([x], None, b, cout, 3, out_amax=slot, defer_stats=True, **kw)
    finally:
        ops.split_k = True
    assert isinstance(pend, PendingStats) and not pend.desc.d_workspace      # unsplit: tile partials
    spatial = out[0].numel()
    old = ops.stats_finalize(pend)
    for mode, groups in ((0, 1), (1, 32)):
        weight = (1 + 0.3 * torch.randn(cout, generator=g)) if mode == 1 else None
        bias = torch.randn(cout, generator=g) if mode == 1 else None
        to = lambda t: t.to(dev) if t is not None else None
        a_old, b_old = ops.norm_finalize(old, spatial, mode, groups=groups, weight=to(weight), bias=to(bias))
        a, bb, sums = ops.stats_norm_finalize([pend], spatial, mode, groups=groups, weight=to(weight), bias=to(bias))
        torch.cuda.synchronize()
        a_ref, b_ref, tol_a, tol_b = _affine_ref([out.double().reshape(cout, -1).cpu()], mode, groups, weight, bias)
        ea, eb = (a.cpu().double() - a_ref).abs(), (bb.cpu().double() - b_ref).abs()
        print(f"mode {mode}: worst |err| / tolerance a {float((ea / tol_a).max()):.2e} b {float((eb / tol_b).max()):.2e}; "
              f"sums == pixie_stats_finalize: {torch.equal(sums[0], old)}; affine == two launches: {torch.equal(a, a_old) and torch.equal(bb, b_old)}")
        assert bool((ea <= tol_a).all()) and bool((eb <= tol_b).all())
        assert bool(((a.cpu().double() - a_old.cpu().double()).abs() <= 2 * tol_a).all())
        assert bool(((bb.cpu().double() - b_old.cpu().double()).abs() <= 2 * tol_b).all())
        o64 = out.double().reshape(cout, -1)
        assert _rel(sums[0][:, 0].cpu(), o64.sum(1).cpu()) < STAT_TOL and _rel(sums[0][:, 1].cpu(), (o64 * o64).sum(1).cpu()) < STAT_TOL
