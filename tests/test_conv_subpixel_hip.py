"""GPU operator tests of the sub-pixel up-convolution (conv3d_f16x3_subpixel_kernel + pixie_conv_pack_weights_subpixel):
the 3^3 convolution behind a nearest x2 upsampling as eight 2x2x2-tap convolutions over the stored tensor.  Same float64
reference (test_unet_hip.ref_conv) and the same bounds as the 27-tap f16x3 operator tests: rel-L2 < 2e-6 against float64,
epilogue statistics < 1e-6 and |x|max bit-equal against a separate pass, split-K < 1e-6 against the unsplit launch."""
import numpy as np
import pytest
import torch

from test_unet_hip import _amax_slots, _prologue_cpu, ref_conv, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


# prologue: False = raw input, True = per-channel norm affine, "ln" = norm affine + spatial LayerNorm gamma/beta of the STORED grid
SUBPIXEL_CASES = [
    # (cin parts, cout, stored dims, prologue, act, residual, out_size)
    ((64,), 64, (16, 16, 16), False, 0, False, None),       # raw input (the network's Upsample.conv), interior tiles, MB2
    ((64,), 64, (32, 32, 32), False, 0, True, None),        # the full-resolution shape at a quarter of the extent, + residual
    ((128,), 128, (4, 4, 4), False, 0, False, None),        # c7 of test_unet_hip: tiny volume, partial tiles
    ((64,), 64, (8, 8, 16), True, 1, False, None),          # norm affine + LeakyReLU prologue
    ((64,), 64, (8, 8, 16), True, 2, True, None),           # norm affine + SiLU prologue, residual
    ((32,), 64, (8, 16, 8), True, 0, False, None),          # norm affine, no activation
    ((64, 64), 64, (8, 8, 8), False, 0, False, None),       # two concatenated inputs
    ((32, 16), 64, (6, 5, 7), True, 1, True, None),         # concat + prologue + residual, odd stored dims
    ((64,), 64, (5, 5, 5), False, 0, False, (9, 9, 9)),     # odd-grid crop (golden odd9)
    ((64,), 64, (7, 7, 7), True, 1, True, (13, 13, 13)),    # odd-grid crop (golden odd13) + prologue + residual
    ((64,), 64, (16, 16, 16), False, 0, True, (31, 32, 31)),  # crop of a volume with interior tiles: last tiles leave the fast epilogue
    ((16,), 64, (1, 1, 1), False, 0, False, None),          # one stored voxel
    ((16,), 64, (2, 2, 2), True, 2, False, None),
    ((16,), 64, (7, 1, 2), False, 0, False, None),
    ((64,), 8, (8, 8, 8), True, 1, False, None),            # c_out 8 -> padded 32: MB1
    ((64,), 32, (16, 16, 16), False, 0, True, None),        # MB1, interior tiles
    ((48,), 40, (5, 7, 9), True, 2, True, None),            # c_out not a multiple of 32
    ((256,), 256, (4, 4, 4), False, 0, True, None),         # deep level (splits its channel chunks)
    ((64,), 64, (16, 16, 16), "ln", 1, False, None),        # LayerNorm affine + LeakyReLU (the network's norm), interior tiles
    ((64,), 64, (32, 32, 32), "ln", 1, True, None),         # the same on 32-wide tiles, + residual
    ((64,), 64, (7, 7, 7), "ln", 1, True, (13, 13, 13)),    # LayerNorm affine, odd-grid crop, partial tiles
    ((32, 16), 64, (6, 5, 7), "ln", 2, False, None),        # LayerNorm affine + SiLU over two inputs, odd stored dims
    ((64,), 8, (5, 8, 9), "ln", 0, False, (9, 16, 17)),     # LayerNorm affine, no activation, MB1, crop
]


def _setup(ops, case, seed):
    cins, cout, dims, prologue, act, has_res, out_size = case
    g = torch.Generator().manual_seed(seed)
    parts = [torch.randn((c,) + dims, generator=g) * (1.0 + 3.0 * i) for i, c in enumerate(cins)]
    cin = sum(cins)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) / np.sqrt(cin * 27)
    b = torch.randn(cout, generator=g)
    pro = (torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)) if prologue else None
    # gamma/beta live on the stored grid: ref_conv applies them before the upsampling, as the kernel does
    affine = (torch.randn(dims, generator=g), torch.randn(dims, generator=g)) if prologue == "ln" else None
    ref = ref_conv(parts, w, b, 1, True, pro, affine, act, None)
    if out_size is not None:
        ref = ref[:, :out_size[0], :out_size[1], :out_size[2]]
    residual = torch.randn(ref.shape, generator=g) if has_res else None
    if has_res:
        ref = ref + residual.double()
    to = lambda t: t.to(ops.device) if t is not None else None
    dparts = [to(p) for p in parts]
    kw = dict(upsample=True, pro=tuple(map(to, pro)) if pro else None, affine=tuple(map(to, affine)) if affine else None,
              act=act, residual=to(residual), subpixel=True)
    if out_size is not None:
        kw["out_size"] = out_size
    if prologue:   # host bound on |prologue(x)|, deliberately loose by 3x: any valid bound must work
        kw["in_bound"] = 3.0 * float(_prologue_cpu(parts, pro, affine, act).abs().max())
    else:
        kw["in_amax"] = _amax_slots(ops, dparts)
    return dparts, to(w), to(b), cout, kw, ref


@pytest.mark.parametrize("case", SUBPIXEL_CASES, ids=[f"s{i}" for i in range(len(SUBPIXEL_CASES))])
def test_subpixel_upconv_operator(ops, case):
    dparts, w, b, cout, kw, ref = _setup(ops, case, 41 + SUBPIXEL_CASES.index(case))
    w16 = ops.pack_conv_subpixel(w)
    out = ops.conv(dparts, None, b, cout, 3, w16=w16, **kw)
    out2 = ops.conv(dparts, None, b, cout, 3, w16=w16, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape)
    err = rel_l2(out.cpu().numpy(), ref.numpy())
    print(f"sub-pixel conv {case}: rel-L2 {err:.3e}")
    assert err < 2e-6, err
    assert torch.equal(out, out2)


STATS_CASES = (0, 1, 4, 6, 7, 9, 10, 14, 16, 18, 20)


@pytest.mark.parametrize("case", [SUBPIXEL_CASES[i] for i in STATS_CASES], ids=[f"s{i}" for i in STATS_CASES])
def test_subpixel_upconv_epilogue_statistics(ops, case):
    """Channel sums / sums of squares / |x|max from the sub-pixel epilogue (four parity workgroups per tile, each with its
    own partials) equal a separate pixie_channel_stats pass over the written tensor."""
    dparts, w, b, cout, kw, ref = _setup(ops, case, 59)
    slot = torch.zeros(1, dtype=torch.int32, device=ops.device)
    ops.split_k = False   # split-K layers leave the statistics to a separate pass
    try:
        out, sums = ops.conv(dparts, None, b, cout, 3, w16=ops.pack_conv_subpixel(w), out_amax=slot, **kw)
    finally:
        ops.split_k = True
    assert sums is not None and tuple(sums.shape) == (cout, 2)
    assert rel_l2(out.cpu().numpy(), ref.numpy()) < 2e-6
    slot2 = torch.zeros(1, dtype=torch.int32, device=ops.device)
    ref_sums = ops.channel_stats(out, slot2)
    err = rel_l2(sums.cpu().numpy(), ref_sums.cpu().numpy())
    print(f"sub-pixel statistics {case}: rel-L2 {err:.3e}")
    assert err < 1e-6
    assert int(slot.item()) == int(slot2.item())   # same float bits
    assert abs(float(slot.view(torch.float32).item()) - float(out.abs().max())) == 0.0


SUBPIXEL_SPLIT_K_SHAPES = [((256,), 256, (8, 8, 8)), ((256,), 256, (16, 16, 16)), ((128, 128), 128, (4, 4, 4))]


@pytest.mark.parametrize("shape", SUBPIXEL_SPLIT_K_SHAPES)
def test_subpixel_upconv_split_k(ops, shape):
    """The deep up-convs have too few tiles for the chip and split their channel chunks: same result as the unsplit
    launch to fp32 summation-order accuracy, bit-reproducible, no epilogue statistics."""
    cins, cout, dims = shape
    dparts, w, b, cout, kw, ref = _setup(ops, (cins, cout, dims, False, 0, True, None), 67)
    w16 = ops.pack_conv_subpixel(w)
    slot = torch.zeros(1, dtype=torch.int32, device=ops.device)
    a, sums = ops.conv(dparts, None, b, cout, 3, w16=w16, out_amax=slot, **kw)
    a2 = ops.conv(dparts, None, b, cout, 3, w16=w16, **kw)
    assert sums is None                      # this shape splits
    assert torch.equal(a, a2)
    ops.split_k = False
    try:
        unsplit = ops.conv(dparts, None, b, cout, 3, w16=w16, **kw)
    finally:
        ops.split_k = True
    assert rel_l2(a.cpu().numpy(), unsplit.cpu().numpy()) < 1e-6
    assert rel_l2(a.cpu().numpy(), ref.numpy()) < 2e-6 and rel_l2(unsplit.cpu().numpy(), ref.numpy()) < 2e-6


def test_subpixel_agrees_with_the_27_tap_form(ops):
    """Both forms of the same layer against float64 and against each other (they differ by summation order only)."""
    dparts, w, b, cout, kw, ref = _setup(ops, SUBPIXEL_CASES[1], 71)
    sub = ops.conv(dparts, None, b, cout, 3, w16=ops.pack_conv_subpixel(w), **kw)
    kw27 = dict(kw, subpixel=False)
    full = ops.conv(dparts, None, b, cout, 3, w16=ops.pack_conv16(w), **kw27)
    e_sub, e_27 = rel_l2(sub.cpu().numpy(), ref.numpy()), rel_l2(full.cpu().numpy(), ref.numpy())
    between = rel_l2(sub.cpu().numpy(), full.cpu().numpy())
    print(f"vs float64: sub-pixel {e_sub:.3e}, 27 taps {e_27:.3e}; between them {between:.3e}")
    assert e_sub < 2e-6 and e_27 < 2e-6
    assert between < 4e-6   # what the two bounds against float64 imply (triangle inequality)


def test_subpixel_weights_are_refused_on_other_layers(ops):
    from pixie_amd._lib import PixieHipError
    g = torch.Generator().manual_seed(3)
    x = torch.randn((16, 4, 4, 4), generator=g).to(ops.device)
    w = torch.randn((32, 16, 3, 3, 3), generator=g).to(ops.device)
    b = torch.zeros(32, device=ops.device)
    with pytest.raises(PixieHipError):   # not an upsampling layer
        ops.conv([x], None, b, 32, 3, w16=ops.pack_conv_subpixel(w), in_amax=_amax_slots(ops, [x]), subpixel=True)
    with pytest.raises(PixieHipError):   # c_in not a multiple of 16
        ops.pack_conv_subpixel(torch.randn((32, 8, 3, 3, 3), generator=g).to(ops.device))
