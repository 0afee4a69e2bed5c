"""The pair form of the f16x3 convolutions (conv3d_f16x3_pair_kernel<KS, 4>: 512 threads, two quartets of 4 waves over ONE tile
and 128 output channels, the tile staged once for both into two LDS buffers) against the 4-wave form of the same plan.

The launcher takes the pair form for unsplit plans on the plain f16x3 path with MB = 2, NB = 4, an even number of 64-channel
blocks, no folded skip and an LDS request within 160 KB; the plan itself (variant number, tile, statistics layout) is the 4-wave
form's.  Measured per class against the 4-wave form (profiles/conv_pair_pricing.txt), the two 128^3 classes cleared the project's
2 % bar and the split-K classes of the 32^3 and 16^3 levels did not, so split launches and NB < 4 keep the 4-wave kernels and
<3,2,4> and <1,2,4> are the pair form's only instantiations; FOUR_WAVE holds one row per class that must stay where it is.

The PIXIE_DIAG build can be told to keep the 4-wave kernels (pixie_conv_kernel_variant with a null descriptor) and says which
form a descriptor gets (pixie_conv_tile_geometry with a null `out`), so every case of CASES runs the SAME descriptor twice through
libpixie_hip_diag.so and requires byte-equal outputs, statistics buffers and |x|max slots: each wave of a quartet is the 4-wave
form's wave, no product order or partial-sum grouping may differ.

CASES: one row per thing that selects code in the pair form, at the smallest shapes at which the planner keeps NB = 4 without
splitting (asserted from pixie_conv_tile_geometry): 512 workgroups of the 4-wave form, e.g. c_out 256 at 32 x 32 x 64.
  chunks      c_in 32 (one buffer swap), 48 (odd count: the last chunk is in buffer 0), 64 (the general loop)
  c_out       128, 256, 100 (c_out padded 128: the second quartet's block is partly padding and takes the plain epilogue beside
              the first quartet's transposing one); 192 (three blocks) is a FOUR_WAVE row
  tiles       interior-only outputs, partial tiles on all three axes (33 x 65 x 65, 33 x 33 x 65), an odd-grid crop behind x2
  epilogue    bias or none x residual or none x statistics or none
  prologue    none / norm / norm + LayerNorm affine, each with LeakyReLU and SiLU
  two inputs  16 | 32 (the second quartet's half holds slots of both tensors' chunks) and 8 | 24 (a chunk of both tensors)
  NaN         element 0 of every plane (and of gamma / beta) is NaN, which is what a slot outside the input loads before the mask;
              the high halo planes lie in the second quartet's half of the slots

REF: one case per instantiation (and the c_out 100 one) is also compared with tests/_torch_ref_ops.TorchRefOps.conv in float64,
at the bounds tests/test_conv_variants_hip.py holds the f16x3 path to (rel-L2 2e-6 over the whole output and on the worst tile)."""
import ctypes as C
import functools
import json
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import test_conv_variants_hip as tvar
from _conv_census import operator_desc, stats_layout, tile_geometry
from _torch_ref_ops import TorchRefOps
from pixie_amd import _lib
from pixie_amd.unet import fill_conv_desc
from test_unet_hip import _amax_slots, _prologue_cpu, rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_conv_plan_table as table      # noqa: E402

LDS_MAX = 160 * 1024

# up: nearest x2 in front (27-tap form); out_size: the odd-grid crop; pro: "none" | "channel" | "channel+spatial"; act 0 / 1 LeakyReLU /
# 2 SiLU; split_k: a workspace is offered; nb, slices: what the plan must answer; pair: the form the launcher must take;
# ref: also compared with the float64 reference; nan: element 0 of every plane is NaN
PC = namedtuple("PC", "id k cins cout dims up out_size pro act bias res stats split_k nb slices pair ref nan")


def _c(id, k, cins, cout, dims, pro, act, bias, res, stats, nb=4, slices=1, split_k=True, pair=True, ref=False, nan=False, up=False,
       out_size=None):
    return PC(id, k, tuple(cins), cout, tuple(dims), up, out_size, pro, act, bias, res, stats, split_k, nb, slices, pair, ref, nan)


CASES = [
    # both instantiations with the float64 reference; c_in 32, 48, 64
    _c("k3-c32-256", 3, (32,), 256, (32, 32, 64), "channel+spatial", 1, True, True, True, ref=True),     # the smallest unsplit <3,2,4>
    _c("k3-c48-256", 3, (48,), 256, (32, 32, 64), "channel", 2, True, False, True),
    _c("k3-c64-256", 3, (64,), 256, (32, 32, 64), "none", 0, False, True, False),
    _c("k1-c32-256", 1, (32,), 256, (32, 32, 64), "channel", 1, False, False, False, ref=True),
    _c("k1-c48-256", 1, (48,), 256, (32, 32, 64), "channel+spatial", 2, True, False, True),
    _c("k1-c64-256", 1, (64,), 256, (32, 32, 64), "none", 2, True, True, True),
    # c_out 128, and c_out 100 over partial tiles on all three axes
    _c("k3-c32-128", 3, (32,), 128, (32, 64, 64), "channel", 2, True, True, True),
    _c("k3-c32-100-ragged", 3, (32,), 100, (33, 65, 65), "none", 1, True, True, True),
    _c("k1-c32-100-ragged", 1, (32,), 100, (33, 65, 65), "channel", 2, True, False, True, ref=True),
    # partial tiles on all three axes with two full blocks, and an odd-grid crop behind the x2 upsampling
    _c("k3-c32-256-ragged", 3, (32,), 256, (33, 33, 65), "channel+spatial", 2, True, True, True),
    _c("k3-c32-128-crop", 3, (32,), 128, (17, 33, 33), "none", 0, True, False, True, up=True, out_size=(33, 65, 65)),
    # the epilogue bodies the rows above leave out
    _c("k1-bias", 1, (32,), 256, (32, 32, 64), "none", 0, True, False, False),
    _c("k1-bias-res", 1, (32,), 256, (32, 32, 64), "none", 0, True, True, False),
    _c("k1-res-stats", 1, (32,), 256, (32, 32, 64), "none", 0, False, True, True),
    _c("k1-stats", 1, (32,), 256, (32, 32, 64), "none", 0, False, False, True),
    # two input tensors
    _c("k3-16+32-256", 3, (16, 32), 256, (32, 32, 64), "channel+spatial", 1, True, True, True),
    _c("k3-8+24-256", 3, (8, 24), 256, (32, 32, 64), "channel", 2, True, False, True),
    # NaN in what the slots outside the input load
    _c("k3-c32-nan", 3, (32,), 256, (33, 33, 65), "channel+spatial", 2, True, False, True, nan=True),
    _c("k1-c32-nan", 1, (32,), 256, (33, 33, 65), "channel", 1, True, False, True, nan=True),
]
IDS = [c.id for c in CASES]
# what keeps the 4-wave kernels (host assertions only: there the switch changes nothing): three 64-channel blocks, NB < 4, split-K
# (the launches of the 32^3 and 16^3 levels among them)
FOUR_WAVE = [
    _c("k3-c32-192", 3, (32,), 192, (32, 48, 64), "channel", 1, True, True, True, pair=False),
    _c("k3nb2-c48-128", 3, (48,), 128, (32, 32, 64), "channel", 2, True, False, True, nb=2, pair=False),
    _c("k3nb1-c64-128", 3, (64,), 128, (16, 32, 64), "none", 0, False, True, False, nb=1, split_k=False, pair=False),
    _c("k1nb2-c64-128", 1, (64,), 128, (32, 32, 64), "none", 2, True, True, True, nb=2, split_k=False, pair=False),
    _c("k1nb1-c48-128", 1, (48,), 128, (16, 32, 64), "channel+spatial", 2, True, False, True, nb=1, pair=False),
    _c("k3nb1-c64-split2", 3, (64,), 128, (9, 5, 33), "channel+spatial", 1, True, True, True, nb=1, slices=2, pair=False),
    _c("k3-c128-split4", 3, (128,), 128, (32, 32, 32), "channel", 2, True, False, True, slices=4, pair=False),
    _c("k3nb2-c256-split8", 3, (256,), 256, (16, 16, 16), "channel+spatial", 1, True, True, False, nb=2, slices=8, pair=False),
    _c("k1-c128-split4", 1, (128,), 128, (32, 32, 32), "channel", 1, False, True, True, slices=4, pair=False),
    _c("k1nb2-c256-split8", 1, (256,), 256, (16, 16, 16), "none", 0, True, False, True, nb=2, slices=8, pair=False),
]


def meta_desc(case):
    """the descriptor of a case from shapes alone (no device), with the statistics asked for as the launch asks"""
    return operator_desc("f16x3", case.cins, case.cout, case.dims, case.k, upsample=case.up, prologue=case.pro, residual=case.res,
                         stats=case.stats, out_size=case.out_size, split_k=case.split_k, split_stats=True)


def launch_form(desc):
    """dynamic LDS bytes of the pair-form launch the launcher gives this descriptor, 0: it keeps the 4-wave kernel"""
    return int(_lib.load(diag=True).pixie_conv_tile_geometry(C.byref(desc), None))


def keep_four_wave(on):
    """the diag build's switch; returns the setting before"""
    v = C.c_int(1 if on else 0)
    return int(_lib.load(diag=True).pixie_conv_kernel_variant(None, C.byref(v)))


def halo_slots(geo, k, stride=1):
    return ((geo["TX"] - 1) * stride + k) * ((geo["TY"] - 1) * stride + k) * ((geo["TZ"] - 1) * stride + k)


def pair_lds_of_plan(geo, k, stride):
    """the pair form's LDS request from the plan's answers: two tile buffers of four 16-byte planes per slot, or the eight waves'
    transposing area and the two quartets' statistics partials where the plan reserved the epilogue's LDS"""
    red = 2 * 4 * geo["MB"] * 32 * 2 * 4
    epi = 8 * 32 * (geo["NB"] * 32 + 4) * 4 + red if geo["epi_lds"] else red
    return max(2 * 64 * halo_slots(geo, k, stride), epi)


def test_the_cases_reach_what_they_are_there_for():
    """(no device) <3,2,4> and <1,2,4> unsplit in pair form, every FOUR_WAVE row on the 4-wave kernels, and the switch"""
    assert keep_four_wave(False) == 0
    for c in CASES + FOUR_WAVE:
        desc, _ = meta_desc(c)
        geo = tile_geometry(desc)
        sl = C.c_int(1)
        variant = int(_lib.load(diag=True).pixie_conv_kernel_variant(C.byref(desc), C.byref(sl)))
        assert (geo["MB"], geo["NB"], geo["slices"]) == (2, c.nb, c.slices) and variant == c.k * 100 + 20 + c.nb and int(sl.value) == c.slices, (c.id, geo, variant)
        lds = launch_form(desc)
        assert (lds > 0) == c.pair and lds <= LDS_MAX, (c.id, lds)
        if c.pair:
            assert lds == pair_lds_of_plan(geo, c.k, 1) and geo["epi_lds"] == 1, (c.id, lds, geo)
        assert keep_four_wave(True) == 0 and launch_form(desc) == 0 and keep_four_wave(False) == 1     # the switch, and back
    assert all(c.pair and c.nb == 4 and c.slices == 1 for c in CASES) and not any(c.pair for c in FOUR_WAVE)
    assert {c.k for c in CASES} == {1, 3}
    assert {(c.k, sum(c.cins)) for c in CASES} >= {(k, n) for k in (1, 3) for n in (32, 48, 64)}          # two, three and four chunks
    assert {c.cout for c in CASES} >= {100, 128, 256} and any(c.cout == 192 and c.nb == 4 and c.slices == 1 for c in FOUR_WAVE)
    assert {(c.pro, c.act) for c in CASES} >= {(p, a) for p in ("none", "channel", "channel+spatial") for a in (1, 2)}
    assert {(c.bias, c.res, c.stats) for c in CASES} == {(b, r, s) for b in (False, True) for r in (False, True) for s in (False, True)}
    assert any(c.cins == (16, 32) for c in CASES) and any(c.cins == (8, 24) for c in CASES)
    assert {c.k for c in CASES if c.nan} == {1, 3} and {c.k for c in CASES if c.ref and c.cout == 256} == {1, 3}
    assert {(c.nb, c.slices > 1) for c in FOUR_WAVE} >= {(4, True), (2, True), (1, True), (2, False), (1, False)}

    def ragged(c):
        desc, oshape = meta_desc(c)
        geo = tile_geometry(desc)
        return all(e % geo[a] != 0 for e, a in zip(oshape[1:], ("TZ", "TY", "TX")))

    assert {c.cout for c in CASES if ragged(c)} >= {100, 256} and any(ragged(c) and c.out_size for c in CASES)
    assert any(not ragged(c) and c.res and c.stats for c in CASES)


def test_the_launch_form_is_a_function_of_the_plan():
    """(no device) For every descriptor of the recorded plan table that pixie_conv3d_forward accepts, the launcher's form follows
    from the plan's own answers -- path, variant, split factor, c_out padded, tile, epi_lds -- and from whether a folded skip rides along; its
    LDS request is within 160 KB; stride-2 tiles, sub-pixel and folded-skip launches and the 64 -> 64 full-resolution kernel keep the
    4-wave form, and so do split-K launches; and no query of the table answers differently (tests/test_conv_plan_table.py holds that, unchanged)."""
    assert keep_four_wave(False) == 0
    with open(table.OUT) as f:
        doc = json.load(f)
    n_pair = n_acc = 0
    by_plan = {}
    for rec in doc["rows"]:
        row = dict(zip(table.COLUMNS, rec))
        if not row["accepted"]:
            continue
        n_acc += 1
        desc = table.descriptor(row)
        lds = launch_form(desc)
        want = 0
        tiled16 = row["w16"] and row["geometry"] is not None and row["variant"] in (324, 124) and row["slices"] == 1
        if tiled16 and not row["skip"] and row["layout"][5] % 128 == 0:
            geo = dict(zip(("TX", "TY", "TZ", "tiles_x", "tiles_y", "tiles_z", "epi_lds", "slices", "MB", "NB"), row["geometry"]))
            assert geo["MB"] == 2
            need = pair_lds_of_plan(geo, row["ksize"], row["stride"])
            want = need if need <= LDS_MAX else 0
        assert lds == want and lds <= LDS_MAX, (lds, want, rec)
        if row["stride"] == 2 or row["subpixel"] or row["skip"] or row["variant"] == 9324 or not row["w16"] or row["slices"] > 1:
            assert lds == 0, rec
        key = (row["variant"], row["slices"], tuple(row["geometry"] or ()), tuple(row["layout"] or ()), row["ksize"], row["stride"], row["w16"], row["skip"])
        assert by_plan.setdefault(key, lds) == lds, rec
        n_pair += lds > 0
    print(f"{n_acc} accepted descriptors, {n_pair} in pair form")
    assert n_acc > 700 and n_pair >= 4


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


@functools.lru_cache(maxsize=1)
def host_case(case):
    """host tensors of a case (seeded), as tests/test_conv_variants_hip.make_case makes them"""
    g = torch.Generator().manual_seed(9100 + CASES.index(case))
    parts = [torch.randn((c,) + case.dims, generator=g) * (1.0 + 3.0 * i) for i, c in enumerate(case.cins)]
    parts[0] += 3.0
    cin = sum(case.cins)
    w = torch.randn((case.cout, cin) + (case.k,) * 3, generator=g) / np.sqrt(cin * case.k ** 3)
    b = (1.0 + torch.randn(case.cout, generator=g).abs()) if case.bias else None
    pro = (torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)) if case.pro != "none" else None
    affine = (torch.randn(case.dims, generator=g), torch.randn(case.dims, generator=g)) if case.pro == "channel+spatial" else None
    oshape = meta_desc(case)[1]
    residual = torch.randn(oshape, generator=g) if case.res else None
    return parts, w, b, pro, affine, residual


def run_form(ops, case, host, four_wave, bound):
    """one launch of the case through the diag library -> (out, raw statistics buffer, |x|max slot), device tensors"""
    parts, w, b, pro, affine, residual = host
    dev = ops.device
    lib = _lib.load(diag=True)
    to = lambda t: t.to(dev) if t is not None else None
    dparts = [to(p) for p in parts]
    kw = dict(upsample=case.up, pro=tuple(map(to, pro)) if pro else None, affine=tuple(map(to, affine)) if affine else None, act=case.act,
              residual=to(residual), w16=ops.pack_conv16(to(w)), out_size=case.out_size, split_k=case.split_k, split_stats=True)
    if bound is not None:
        kw["in_bound"] = bound
    else:
        kw["in_amax"] = _amax_slots(ops, dparts)
    slot = torch.zeros(1, dtype=torch.int32, device=dev) if case.stats else None
    zeros = lambda shape, dtype: torch.zeros(shape, device=dev, dtype=dtype)      # every byte compared is one the launch wrote, or zero
    desc, out, stats, workspace = fill_conv_desc(lib, zeros, dparts, None, to(b), case.cout, case.k, out_amax=slot, **kw)
    geo = tile_geometry(desc)
    assert (geo["MB"], geo["NB"], geo["slices"]) == (2, case.nb, case.slices), (case.id, geo)
    assert workspace is None and (stats is not None) == case.stats
    before = keep_four_wave(four_wave)
    try:
        assert (launch_form(desc) > 0) == (case.pair and not four_wave), case.id
        _lib.check(lib.pixie_conv3d_forward(C.byref(desc), _lib.current_stream_ptr()), "pixie_conv3d_forward")
        torch.cuda.synchronize()
    finally:
        keep_four_wave(bool(before))
    return out, stats, slot


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pair_form_equals_four_wave_form(ops, case):
    host = host_case(case)
    parts, w, b, pro, affine, residual = host
    clean = None
    if case.nan:     # what a slot outside the input loads, made NaN; the bound comes from the clean tensors (no amax pass sees the NaN)
        clean = ([p.clone() for p in parts], tuple(a.clone() for a in affine) if affine else None)
        for p in clean[0]:
            p[:, 0, 0, 0] = 0.0
        for p in parts:
            p[:, 0, 0, 0] = float("nan")
        for a in (clean[1] or ()):
            a[0, 0, 0] = 0.0
        for a in (affine or ()):
            a[0, 0, 0] = float("nan")
    bound = None
    if pro is not None or affine is not None or case.nan:
        src = (clean[0], clean[1]) if case.nan else (parts, affine)
        bound = 3.0 * float(_prologue_cpu(src[0], pro, src[1], case.act).abs().max())
    try:
        pair = run_form(ops, case, host, False, bound)
        four = run_form(ops, case, host, True, bound)
    finally:
        if case.nan:     # host_case is cached: put the planted elements back
            for p, q in zip(parts, clean[0]):
                p[:, 0, 0, 0] = q[:, 0, 0, 0]
            for a, q in zip(affine or (), clean[1] or ()):
                a[0, 0, 0] = q[0, 0, 0]
    for what, x, y in zip(("output", "statistics", "|x|max"), pair, four):
        assert (x is None) == (y is None), what
        if x is not None:
            assert same_bytes(x, y), f"{case.id}: {what} differ between the pair and the 4-wave form"
    out = pair[0].cpu().numpy()
    if case.nan:
        pad = 1 if case.k == 3 else 0
        sees = np.zeros(out.shape, bool)
        sees[:, :pad + 1, :pad + 1, :pad + 1] = True       # the outputs whose receptive field holds voxel (0, 0, 0)
        assert np.isfinite(out[~sees]).all(), f"{int((~np.isfinite(out[~sees])).sum())} non-finite outputs that cannot see voxel (0, 0, 0)"
    else:
        assert np.isfinite(out).all()
    if not case.ref:
        return
    d64 = lambda t: t.double() if t is not None else None
    ref = TorchRefOps().conv([d64(p) for p in parts], d64(w), d64(b), case.cout, case.k, 1, case.up, tuple(map(d64, pro)) if pro else None,
                             tuple(map(d64, affine)) if affine else None, case.act, d64(residual), out_size=case.out_size).numpy()
    geo = tile_geometry(meta_desc(case)[0])
    whole, worst = rel_l2(out, ref), tvar.per_tile_rel_l2(out, ref, geo["TZ"], geo["TY"], geo["TX"])
    print(f"{case.id} <{case.k},2,{case.nb}>: rel-L2 whole {whole:.3e}, worst tile {worst:.3e}")
    assert whole < tvar.TOL["f16x3"], whole
    assert worst < tvar.PER_TILE_TOL["f16x3"], worst
    if case.stats:
        # the tile partials, added up, against the float64 reference: the sum of squares, which cannot cancel, at test_conv_variant's
        # bound (the sum's relative error is the channel's condition number where a mean cancels: see that module's docstring)
        lay = stats_layout(meta_desc(case)[0])
        s = pair[1].cpu().double().reshape(lay["n"], lay["coutp"], 2)[:, :case.cout].sum(0)
        r64 = torch.from_numpy(ref).reshape(case.cout, -1)
        assert torch.allclose(s[:, 1], (r64 * r64).sum(1), rtol=1e-5)
        assert float(pair[2].view(torch.float32).item()) == float(pair[0].abs().max())
