"""GPU tests of the statistics a split-K launch takes in its reduce, and of the merged finalise (pixie_stats_norm_finalize).

A split-K layer's slices are added by a reduce kernel.  Asked for statistics (pixie_conv_desc.d_out_stats, HipOps.conv with
defer_stats), that kernel also leaves per channel and segment the sum and the sum of squares of the values it stores, in
float64, and the tensor's |x|max; pixie_stats_finalize / pixie_stats_norm_finalize add the segments up.  The rows of REDUCE_ROWS
and FINALISE_ROWS are plain data (no device needed to import them): tests/test_conv_variant_census.py reads them and asks for a
row per reduce class and finalise class the networks launch.  Checked here:

* sums and sums of squares against float64 sums of the RETURNED tensor.  Float64 segment partials: absolute error per channel
  <= 4 osp 2^-53 sum|x| (sum) and <= 4 osp 2^-53 sum x^2 (squares), osp the voxels per channel: float64 summation of osp terms in
  any order errs by at most (osp - 1) 2^-53 sum|x|, the reference's own sum by as much, and the square of a float32 is exact in
  float64.  One voxel dropped or counted twice moves a sum by about the mean |x|, 2^53 / (4 osp^2) bounds: 3e4 at 64^3 outputs
  (tests/test_conv_variant_census.py::test_float64_bound_holds_for_the_reference_alone).  Float32 tile
  partials (unsplit producers): relative error per channel < 1e-5, the bound of the epilogue-statistics tests.
* every slot of the buffer, viewed as float64 [c_out][segments][2], against the float64 sums of its own segment of voxels
  (segment length from pixie_conv_stats_layout), same bound with the segment length for osp;
* |x|max bit-equal, and max(preload, |x|max) bit-equal where the slot held a value before;
* the output is bit-equal to the reduce without statistics (same slice order, then bias, then residual), and two launches
  agree bit for bit in the output and in the sums;
* nothing relies on a zeroed buffer: launched into NaN with a canary tail, no NaN is left and the tail is intact, and a second
  launch with other inputs into the same buffer equals a launch into a fresh one bit for bit;
* a channel that is constant and one that is zero: exact sums, finite affine;
* the merged finalise against the two-launch route (pixie_stats_finalize + pixie_norm_finalize) and against float64.

Bias sign rule (tests/test_conv_variants_hip.py): the bias of a channel, magnitude 1 + |N(0,1)|, has the sign of that channel's
mean output, so that no channel's sum cancels and the relative error of a sum speaks about the summation.  The sign is taken
from a launch with zero bias; it only conditions the data and is no reference.

Tolerance of the affine (a, b), from float64 reference values only.  With m = mean, q = mean of squares, v = q - m^2 of the
float64 reference and e = 1e-5 the relative bound on the two sums: |dm| <= e |m|, |dv| <= e (q + 2 m^2), a = (v + eps)^-1/2 so
|da| <= a |dv| / (2 (v + eps)), and b = -m a (times the weight, plus the bias) so |db| <= |w| (|m| |da| + a |dm|); one float32
rounding (2^-23 relative) is added to each.

Measured on an MI355X, worst over all rows, as a part of the bound it sits under: channel sums from float64 segment partials 7.9e-3
of 4 osp 2^-53 sum|x|; single [c][segment] slots 7.9e-3 of the same bound with the segment length; channel sums from float32 tile
partials 7.0e-3 of 1e-5 (7.0e-8 relative); the affine 1.1e-2 (a) and 1.9e-1 (b) of its tolerance, merged and two-launch route
alike (bit-equal in every row).  The whole file: 5.4 s for 81 of its 83 tests (the 17 before: 2.6 s)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from _conv_census import stats_layout
from test_conv_subpixel_hip import SUBPIXEL_SPLIT_K_SHAPES
from test_unet_hip import SPLIT_K_SHAPES, _amax_slots

pytestmark = pytest.mark.gpu

STAT_TOL = 1e-5
U64 = 2.0 ** -53

# One HipOps.conv call that leaves statistics behind.  sub: sub-pixel up-conv (dims are the stored tensor's); out_size: the
# odd-grid crop; split_k False: HipOps.split_k is off for the launch (an unsplit launch of a shape that would split otherwise).
Prod = namedtuple("Prod", "cins cout dims k sub res out_size split_k")


def P(cins, cout, dims, k=3, sub=False, res=False, out_size=None, split_k=True):
    return Prod(tuple(cins), cout, tuple(dims), k, sub, res, out_size, split_k)


def _shape_id(cins, cout, dims):
    return f"{'+'.join(map(str, cins))}to{cout}-{'x'.join(map(str, dims))}"


# (id, producer): every one must split.  The census names the product's reduce class a row stands for.
REDUCE_ROWS = (
    [(f"k{k}-{_shape_id(cins, cout, dims)}", P(cins, cout, dims, k)) for cins, cout, dims, k in SPLIT_K_SHAPES]
    + [(f"sub-{_shape_id(cins, cout, dims)}", P(cins, cout, dims, 3, sub=True)) for cins, cout, dims in SUBPIXEL_SPLIT_K_SHAPES]
    + [("res-128to128-32x32x32", P((128,), 128, (32, 32, 32), res=True)),
       ("res-256to256-16x16x16", P((256,), 256, (16, 16, 16), res=True)),
       ("res-256to256-5x5x5", P((256,), 256, (5, 5, 5), res=True)),      # odd extent: the scalar form of the reduce
       # the odd-grid networks' layers (golden_odd9, golden_odd13): scalar form, one ragged segment, 2 slices and more
       ("odd5-64to64", P((64,), 64, (5, 5, 5))),
       ("odd5-res-64to64", P((64,), 64, (5, 5, 5), res=True)),
       ("odd7-64+64to64", P((64, 64), 64, (7, 7, 7))),
       ("odd7-pw-64+32to64", P((64, 32), 64, (7, 7, 7), k=1)),
       ("sub-odd-64to64-4to7", P((64,), 64, (4, 4, 4), sub=True, out_size=(7, 7, 7))),     # up-conv with the odd crop
       ("sub-odd-64to64-5to9", P((64,), 64, (5, 5, 5), sub=True, out_size=(9, 9, 9))),
       # 4^3 (golden_odd13's deepest level): vector form, 64 voxels of one segment
       ("k3-64to64-4x4x4", P((64,), 64, (4, 4, 4))),
       ("res-64to64-4x4x4", P((64,), 64, (4, 4, 4), res=True)),
       # two slices, and the residual cases of the 8^3 / 32^3 levels
       ("k3-64to128-16x16x16", P((64,), 128, (16, 16, 16))),
       ("res-256to256-8x8x8", P((256,), 256, (8, 8, 8), res=True)),
       ("k3-64to64-32x32x32", P((64,), 64, (32, 32, 32))),
       ("res-64to64-32x32x32", P((64,), 64, (32, 32, 32), res=True)),
       # the concatenating layers of the 128^3 network (unequal parts)
       ("k3-256+128to128-32x32x32", P((256, 128), 128, (32, 32, 32))),
       ("k3-128+64to64-32x32x32", P((128, 64), 64, (32, 32, 32))),
       # no network has these; the API does: several segments with a ragged last one, in the scalar and in the vector form
       ("res-256to256-17x17x17", P((256,), 256, (17, 17, 17), res=True)),
       ("k3-128to128-20x20x20", P((128,), 128, (20, 20, 20)))])
REDUCE_CASES = [pytest.param(prod, id=rid) for rid, prod in REDUCE_ROWS]
# More than 256 segments per channel would need a split launch with more than 256 * 4096 output voxels.  No legal descriptor
# splits there: a launch splits only where it has fewer than 512 workgroups, and a tile holds at most 512 output voxels.
# tests/test_conv_variant_census.py::test_no_descriptor_splits_beyond_256_segments asks the library.
UNREACHABLE_REDUCE = {"segments>256": "a launch with more than 256 * 4096 output voxels has at least 2048 workgroups and never splits"}


def reduce_row_launches(prod):
    """[(split_k, statistics in the reduce)] of the HipOps.conv calls the tests here make for a producer: what the census counts"""
    return [(prod.split_k, False), (prod.split_k, True)]       # zero-bias and plain launch; the launch with defer_stats


class Producer:
    """The operands of one row, on the device, with the bias chosen by the sign rule.  `special`: {channel: bias} of output
    channels whose weights are zeroed (the channel is then constant: its bias)."""

    def __init__(self, ops, prod, seed, special=None):
        self.ops, self.prod = ops, prod
        g = torch.Generator().manual_seed(seed)
        dev = ops.device
        cins, cout, dims, k = prod.cins, prod.cout, prod.dims, prod.k
        self.parts = [(torch.randn((c,) + dims, generator=g) * (4.0 if i else 1.0)).to(dev) for i, c in enumerate(cins)]
        cin = sum(cins)
        w = torch.randn((cout, cin, k, k, k), generator=g) / np.sqrt(cin * k ** 3)
        bmag = 1.0 + torch.randn(cout, generator=g).abs()
        self.odims = tuple(prod.out_size) if prod.out_size else (tuple(2 * d for d in dims) if prod.sub else dims)
        self.res = torch.randn((cout,) + self.odims, generator=g).to(dev) if prod.res else None
        for ch in (special or {}):
            w[ch] = 0.0
        w = w.to(dev)
        self.kw = dict(w16=ops.pack_conv_subpixel(w) if prod.sub else ops.pack_conv16(w), in_amax=_amax_slots(ops, self.parts),
                       residual=self.res)
        if prod.sub:
            self.kw.update(upsample=True, subpixel=True)
        if prod.out_size:
            self.kw["out_size"] = tuple(prod.out_size)
        zero = self._conv(torch.zeros(cout, device=dev))
        mean = zero.double().reshape(cout, -1).mean(1).cpu()
        b = torch.where(mean < 0, -bmag, bmag)              # the bias sign rule
        for ch, v in (special or {}).items():
            b[ch] = v
        self.b = b.to(dev)

    def _conv(self, bias, **more):
        ops = self.ops
        old = ops.split_k
        ops.split_k = old and self.prod.split_k
        try:
            return ops.conv(self.parts, None, bias, self.prod.cout, self.prod.k, **self.kw, **more)
        finally:
            ops.split_k = old

    def plain(self):
        """the launch without statistics (a split launch: splitk_reduce_kernel)"""
        return self._conv(self.b)

    def with_stats(self, preload=0):
        """-> (out, PendingStats, |x|max slot); the slot holds the int32 `preload` before the launch"""
        from pixie_amd.unet import PendingStats
        slot = torch.full((1,), int(preload), dtype=torch.int32, device=self.ops.device)
        out, pend = self._conv(self.b, out_amax=slot, defer_stats=True)
        assert isinstance(pend, PendingStats), "this shape must leave partial statistics behind"
        return out, pend, slot

    def into(self, make_stats):
        """The same launch as with_stats, the statistics buffer coming from make_stats(floats) -> tensor of that many floats
        -> (out, PendingStats, slot, workspace)"""
        from pixie_amd._lib import check
        from pixie_amd.unet import PendingStats, fill_conv_desc
        ops, prod = self.ops, self.prod
        slot = torch.zeros(1, dtype=torch.int32, device=ops.device)

        def alloc(shape, dtype):
            if dtype == torch.float32 and len(shape) == 1:         # the statistics buffer (the output is 4-d, the workspace bytes)
                return make_stats(int(shape[0]))
            return torch.empty(shape, device=ops.device, dtype=dtype)

        desc, out, stats, ws = fill_conv_desc(ops.lib, alloc, self.parts, None, self.b, prod.cout, prod.k, out_amax=slot,
                                              split_k=ops.split_k and prod.split_k, split_stats=True, **self.kw)
        assert stats is not None
        check(ops.lib.pixie_conv3d_forward(C.byref(desc), ops.stream), "pixie_conv3d_forward")
        return out, PendingStats(stats, desc, prod.cout), slot, ws


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


def _rel(got, ref):
    return float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())


def sum_bounds(x64, n=None):
    """(bound of the sum, bound of the sum of squares) per row of a float64 (rows, n) tensor whose values are float32 values"""
    n = x64.shape[-1] if n is None else n
    return 4.0 * n * U64 * x64.abs().sum(-1), 4.0 * n * U64 * (x64 * x64).sum(-1)


def check_sums(sums, out, f64, what):
    """(c, 2) sums against float64 of the returned tensor: the float64 bound for segment partials, 1e-5 relative for tile
    partials.  Returns the worst error relative to its bound."""
    o64 = out.double().reshape(out.shape[0], -1)
    r1, r2 = o64.sum(1), (o64 * o64).sum(1)
    s = sums.to(o64.device)
    assert tuple(s.shape) == (out.shape[0], 2)
    if f64:
        b1, b2 = sum_bounds(o64)
        e1, e2 = (s[:, 0] - r1).abs(), (s[:, 1] - r2).abs()
        worst = max(float((e1 / b1.clamp_min(1e-300)).max()), float((e2 / b2.clamp_min(1e-300)).max()))
        print(f"{what}: float64 partials, worst |err| / bound {worst:.2e} (bound 4 osp 2^-53 sum|x|, osp = {o64.shape[1]})")
        assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), (float(e1.max()), float(e2.max()))
        rel1, rel2 = _rel(s[:, 0], r1), _rel(s[:, 1], r2)
        assert rel1 < STAT_TOL and rel2 < STAT_TOL, (rel1, rel2)          # the earlier bound, implied wherever no sum cancels
    else:
        e1, e2 = _rel(s[:, 0], r1), _rel(s[:, 1], r2)
        worst = max(e1, e2) / STAT_TOL
        print(f"{what}: float32 tile partials, worst relative error / 1e-5 {worst:.2e}")
        assert e1 < STAT_TOL and e2 < STAT_TOL, (e1, e2)
    return worst


def check_slots(pend, out):
    """every [c][segment] slot of a split launch's statistics against the float64 sums of its own voxels"""
    lay = stats_layout(pend.desc)
    assert lay["f64"] == 1 and lay["cstride"] == lay["n"] and lay["tstride"] == 1, lay
    cout, n, seg = out.shape[0], lay["n"], lay["segment"]
    o64 = out.double().reshape(cout, -1)
    osp = o64.shape[1]
    assert n == -(-osp // seg) and pend.stats.numel() == cout * n * 4, (lay, osp, pend.stats.numel())
    pad = torch.zeros((cout, n * seg), dtype=torch.float64, device=o64.device)
    pad[:, :osp] = o64
    pad = pad.reshape(cout, n, seg)
    slots = pend.stats.view(torch.float64).reshape(cout, n, 2)
    b1, b2 = sum_bounds(pad, min(seg, osp))
    e1, e2 = (slots[..., 0] - pad.sum(-1)).abs(), (slots[..., 1] - (pad * pad).sum(-1)).abs()
    worst = max(float((e1 / b1.clamp_min(1e-300)).max()), float((e2 / b2.clamp_min(1e-300)).max()))
    print(f"slots [c_out {cout}][segments {n}][2]: worst |err| / bound {worst:.2e}")
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), (float(e1.max()), float(e2.max()))


def _bits(t):
    return int(t.view(torch.int32).item())


@pytest.mark.parametrize("prod", REDUCE_CASES)
def test_splitk_reduce_statistics(ops, prod):
    p = Producer(ops, prod, 211)
    cout = prod.cout
    out, pend, slot = p.with_stats()
    assert pend.desc.d_workspace, "this shape must split"
    sums = ops.stats_finalize(pend)
    out2, pend2, slot2 = p.with_stats()
    sums2 = ops.stats_finalize(pend2)
    parent = p.plain()                                    # the reduce without statistics: splitk_reduce_kernel
    torch.cuda.synchronize()
    assert tuple(out.shape) == (cout,) + tuple(p.odims)
    check_sums(sums, out, True, "reduce statistics against float64 of the returned tensor")
    check_slots(pend, out)
    assert float(slot.view(torch.float32).item()) == float(out.abs().max())      # |x|max, same float bits
    assert torch.equal(out, parent)                       # same slice order, same bias and residual order
    assert torch.equal(out, out2) and torch.equal(sums, sums2) and int(slot.item()) == int(slot2.item())
    assert torch.equal(pend.stats.view(torch.int32), pend2.stats.view(torch.int32))


@pytest.mark.parametrize("prod", REDUCE_CASES)
def test_reduce_needs_no_zeroed_buffer(ops, prod):
    """The reduce overwrites every slot it claims and nothing else: launched into NaN with a canary tail; then once more with
    other inputs into the same buffer, against a launch into a fresh buffer."""
    tail, canary = 64, -12345.5
    held = []

    def make(nfl):
        buf = torch.empty(nfl + tail, dtype=torch.float32, device=ops.device)
        buf[:nfl].view(torch.float64).fill_(float("nan"))      # NaN as the float64 the reduce writes (two float32 NaNs read as one
        buf[nfl:] = canary                                     # float64 are a finite number)
        assert bool(torch.isnan(buf[:nfl].view(torch.float64)).all())
        held.append(buf)
        return buf[:nfl]

    first, second = Producer(ops, prod, 211), Producer(ops, prod, 223)
    out, pend, slot, ws = first.into(make)
    buf = held[0]
    nfl = buf.numel() - tail
    assert nfl == ops.lib.pixie_conv_stats_floats(C.byref(pend.desc)) and pend.desc.d_workspace
    sums = ops.stats_finalize(pend)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(buf[:nfl].view(torch.float64)).any()), "a slot of the claimed range was not written"
    assert bool((buf[nfl:] == canary).all()), "written past pixie_conv_stats_floats floats"
    check_sums(sums, out, True, "into a NaN-filled buffer")
    check_slots(pend, out)
    assert float(slot.view(torch.float32).item()) == float(out.abs().max())
    # the same buffer again, other inputs
    out_b, pend_b, slot_b, ws_b = second.into(lambda n: buf[:n])
    fresh_out, fresh, fresh_slot = second.with_stats()
    torch.cuda.synchronize()
    assert torch.equal(out_b, fresh_out) and int(slot_b.item()) == int(fresh_slot.item())
    assert torch.equal(buf[:nfl].view(torch.int32), fresh.stats.view(torch.int32)), "a slot kept something of the launch before"
    assert bool((buf[nfl:] == canary).all())
    assert not torch.equal(out, out_b)


AMAX_ROWS = ("k3-256to256-16x16x16", "res-128to128-32x32x32", "odd5-res-64to64", "res-256to256-17x17x17", "res-64to64-4x4x4",
             "k3-128to128-20x20x20")


@pytest.mark.parametrize("rid", AMAX_ROWS)
def test_reduce_amax_slot_only_grows(ops, rid):
    """The |x|max slot ends as max(what it held, |x|max), bit for bit: held 0, less, exactly |x|max, more."""
    p = Producer(ops, dict(REDUCE_ROWS)[rid], 211)
    out, _, slot = p.with_stats()
    true = out.abs().max().reshape(1)
    assert _bits(slot) == _bits(true) and _bits(true) > 0
    for name, pre in (("less", true * 0.5), ("equal", true.clone()), ("more", true * 2.0), ("one ulp more", None), ("one ulp less", None)):
        bits = _bits(pre) if pre is not None else _bits(true) + (1 if name == "one ulp more" else -1)
        _, _, s = p.with_stats(preload=bits)
        print(f"slot held {name}: {bits:#x} -> {int(s.item()):#x} (|x|max {_bits(true):#x})")
        assert int(s.item()) == max(bits, _bits(true)), name


# (id, producer, sums of the partials are float64): a split vector-form launch with several segments, a scalar-form one, an unsplit one
CONSTANT_ROWS = [("split-128to128-32x32x32", P((128,), 128, (32, 32, 32)), True), ("split-64to64-5x5x5", P((64,), 64, (5, 5, 5)), True),
                 ("tiles-64to64-32x32x32", P((64,), 64, (32, 32, 32), split_k=False), False)]
# channel -> bias of the channels without weights: 1.75 (every sum exact in float64), zero (the channel is all zero), and a
# bias with a full float32 mantissa (its sum exact, its squares rounded: the variance may come out below zero)
CONSTANT_BIAS = {1: 1.75, 2: 0.0, 5: 1.2345678}


@pytest.mark.parametrize("rid,prod,f64", [pytest.param(*r, id=r[0]) for r in CONSTANT_ROWS])
def test_constant_and_zero_channels(ops, rid, prod, f64):
    p = Producer(ops, prod, 227, special=CONSTANT_BIAS)
    cout = prod.cout
    out, pend, slot = p.with_stats()
    assert bool(pend.desc.d_workspace) == f64
    sums = ops.stats_finalize(pend).cpu()
    osp = out[0].numel()
    o = out.reshape(cout, -1)
    for ch, v in CONSTANT_BIAS.items():
        bv = float(np.float32(v))
        assert bool((o[ch] == bv).all()), ch
        if f64 or ch != 5:      # exact: osp * a float32 fits float64 (a float32 tile partial of the full-mantissa bias may round)
            assert float(sums[ch, 0]) == osp * bv, (ch, float(sums[ch, 0]), osp * bv)
    assert float(sums[1, 1]) == osp * 1.75 ** 2 and float(sums[2, 1]) == 0.0
    assert float(slot.view(torch.float32).item()) == float(out.abs().max()) and float(out.abs().max()) > 1.75
    check_sums(sums, out, f64, "with constant channels")
    g = torch.Generator().manual_seed(7)
    for mode, groups in ((0, 1), (1, 32)):
        weight = (1 + 0.3 * torch.randn(cout, generator=g)) if mode == 1 else None
        bias = torch.randn(cout, generator=g) if mode == 1 else None
        to = lambda t: t.to(ops.device) if t is not None else None
        _, pend_m, _ = p.with_stats()
        a, b, sm = ops.stats_norm_finalize([pend_m], osp, mode, groups=groups, weight=to(weight), bias=to(bias))
        torch.cuda.synchronize()
        assert torch.equal(sm[0].cpu(), sums)
        a_ref, b_ref, tol_a, tol_b = _affine_ref([out.double().reshape(cout, -1).cpu()], mode, groups, weight, bias)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        ea, eb = (a.cpu().double() - a_ref).abs(), (b.cpu().double() - b_ref).abs()
        print(f"mode {mode}: worst |err| / tolerance a {float((ea / tol_a).max()):.2e} b {float((eb / tol_b).max()):.2e}; "
              f"a of the constant channels {[float(a[ch]) for ch in CONSTANT_BIAS]}")
        assert bool((ea <= tol_a).all()) and bool((eb <= tol_b).all())
        if mode == 0:
            for ch in (CONSTANT_BIAS if f64 else (1, 2)):       # variance 0 (clamped where it rounds below): a = eps^-1/2
                assert abs(float(a[ch]) - 1e-5 ** -0.5) <= 1e-5 ** -0.5 * 1e-4, (ch, float(a[ch]))


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
    w = weight.double() if (mode == 1 and weight is not None) else torch.ones(c, dtype=torch.float64, device=x.device)
    bb = bias.double() if (mode == 1 and bias is not None) else torch.zeros(c, dtype=torch.float64, device=x.device)
    a, b = rstd * w, bb - m * rstd * w
    dm, dv = STAT_TOL * m.abs(), STAT_TOL * (q + 2 * m * m)
    da = rstd * dv / (2 * (v + eps))
    f32 = 2.0 ** -23
    tol_a = w.abs() * da + f32 * a.abs()
    tol_b = w.abs() * (m.abs() * da + rstd * dm) + f32 * (b.abs() + bb.abs())
    return a, b, tol_a, tol_b


# The producers of a finalise's parts.  Final(p): that part's sums are final already (taken by pixie_stats_finalize beforehand).
Final = namedtuple("Final", "prod")
SPLIT = P((256,), 256, (16, 16, 16), res=True)
SPLIT128 = P((128,), 128, (16, 16, 16))                          # with SPLIT: the 256+128 concatenation of the 128^3 network
SEG8, SEG8_64 = P((128,), 128, (32, 32, 32), res=True), P((64,), 64, (32, 32, 32))      # eight segments per channel
TILES512, TILES512B = P((64,), 64, (64, 64, 64)), P((64,), 64, (64, 64, 64), res=True)  # unsplit at 64^3: 512 tile partials
TILES4096 = P((32,), 32, (128, 128, 128), k=1)                   # a 128^3 producer: 4096 tile partials per channel
HEAD512 = P((64,), 8, (64, 64, 64))                              # c_out 8 padded to 32: tstride = 32, 512 tile partials
UP9, SKIP9 = P((64,), 64, (5, 5, 5), sub=True, out_size=(9, 9, 9)), P((32,), 32, (9, 9, 9))   # golden_odd9's last concatenation
PAD40 = P((64,), 40, (8, 8, 8), split_k=False)                   # c_out 40 padded to 64, 2 tile partials
SEG1_8 = P((256,), 256, (8, 8, 8))
# the producer of test_merged_finalise_of_tile_partials and its (mode, groups)
TILE_PRODUCER, TILE_MODES = P((64,), 64, (32, 32, 32), split_k=False), ((0, 1), (1, 32))
FINALISE_ROWS = [
    ("layernorm-split", (SPLIT,), 0, 1),
    ("groupnorm32-split", (SPLIT,), 1, 32),
    ("layernorm-cat-both-pending", (SPLIT, SPLIT), 0, 1),
    ("layernorm-cat-second-final", (SPLIT, Final(SPLIT)), 0, 1),
    ("groupnorm32-cat-first-final", (Final(SPLIT), SPLIT), 1, 32),
    # more than 256 float32 tile partials per channel: the t += 256 loop of block_channel_sums
    ("layernorm-tiles512", (TILES512,), 0, 1),
    ("groupnorm32-tiles512", (TILES512,), 1, 32),
    ("layernorm-cat-tiles512-final", (TILES512, Final(TILES512B)), 0, 1),
    ("layernorm-cat-tiles512-both", (TILES512, TILES512B), 0, 1),
    ("layernorm-tiles4096-128cubed", (TILES4096,), 0, 1),
    ("layernorm-tiles512-padded", (HEAD512,), 0, 1),
    # the concatenations of the 128^3 network with unequal parts, one and eight segments per channel
    ("layernorm-cat-256+128", (SPLIT, SPLIT128), 0, 1),
    ("layernorm-cat-128+64-segments8", (SEG8, SEG8_64), 0, 1),
    # mixed kinds: float64 segment partials of one layout and float32 tile partials of another, unequal widths
    ("layernorm-cat-segments-tiles-odd9", (UP9, SKIP9), 0, 1),
    ("layernorm-cat-tiles-final-odd9", (SKIP9, Final(UP9)), 0, 1),
    ("layernorm-cat-padded-tiles-segments", (PAD40, SEG1_8), 0, 1),
    ("groupnorm8-padded-tiles", (PAD40,), 1, 8),
    # no network has it; the API does: 384 channels in 32 groups of 12, the group of channels 252..263 straddles c0 = 256
    ("groupnorm32-cat-256+128-straddle", (SPLIT, SPLIT128), 1, 32),
    ("groupnorm8-cat-padded-tiles-segments-straddle", (PAD40, SEG1_8), 1, 8),      # 296 channels in 8 groups of 37
]
FINALISE_CASES = [pytest.param(prods, mode, groups, id=fid) for fid, prods, mode, groups in FINALISE_ROWS]
# float64 segment partials with more than 256 per channel: see UNREACHABLE_REDUCE
UNREACHABLE_FINALISE = {"segment>256": UNREACHABLE_REDUCE["segments>256"]}


@pytest.mark.parametrize("producers,mode,groups", FINALISE_CASES)
def test_merged_finalise(ops, producers, mode, groups):
    """One launch from the producers' partials to (sums, a, b) against the two-launch route and float64."""
    dev = ops.device
    outs, ents, old_sums, f64 = [], [], [], []
    for i, prod in enumerate(producers):
        final = isinstance(prod, Final)
        p = Producer(ops, prod.prod if final else prod, 307 + i)
        out, pend, _ = p.with_stats()
        sums = ops.stats_finalize(pend)
        outs.append(out); old_sums.append(sums); f64.append(bool(pend.desc.d_workspace))
        ents.append(sums.clone() if final else pend)
    c = sum(o.shape[0] for o in outs)
    spatial = outs[0][0].numel()
    assert all(o[0].numel() == spatial for o in outs)
    g = torch.Generator().manual_seed(5)
    weight = (1 + 0.3 * torch.randn(c, generator=g)) if mode == 1 else None
    bias = torch.randn(c, generator=g) if mode == 1 else None
    to = lambda t: t.to(dev) if t is not None else None
    a_old, b_old = ops.norm_finalize(torch.cat(old_sums, 0), spatial, mode, groups=groups, weight=to(weight), bias=to(bias))
    a, b, sums = ops.stats_norm_finalize(ents, spatial, mode, groups=groups, weight=to(weight), bias=to(bias))
    torch.cuda.synchronize()
    for i, (o, sm, old) in enumerate(zip(outs, sums, old_sums)):
        check_sums(sm, o, f64[i], f"merged finalise sums of part {i}")
        assert torch.equal(sm, old)                       # the same additions in the same order as pixie_stats_finalize
    a_ref, b_ref, tol_a, tol_b = _affine_ref([o.double().reshape(o.shape[0], -1) for o in outs], mode, groups, to(weight), to(bias))
    a_ref, b_ref, tol_a, tol_b = a_ref.cpu(), b_ref.cpu(), tol_a.cpu(), tol_b.cpu()
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
    (cin,), cout, dims = TILE_PRODUCER.cins, TILE_PRODUCER.cout, TILE_PRODUCER.dims
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
    for mode, groups in TILE_MODES:
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
