"""The algebra behind the sub-pixel up-convolutions (conv_pack_kernels.h, pack_weights_subpixel_kernel), in float64 on the CPU:
a 3^3 convolution (padding 1) of a nearest-x2 upsampled tensor equals eight 2x2x2-tap convolutions of the STORED tensor, one
per output parity, with the taps that read the same stored voxel summed beforehand.  Pins the tap grouping, the tap origin
per parity, the zero padding and the odd-grid crop."""
import pytest
import torch
import torch.nn.functional as F

# per axis: output parity p, effective tap e -> the original taps (index 0..2 = offset -1..1) that read stored voxel i - 1 + p + e
GROUPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def subpixel_weights(w):
    """(c_out, c_in, 3, 3, 3) -> (2, 2, 2, c_out, c_in, 2, 2, 2): [pz][py][px] parity, then the summed 2x2x2 taps"""
    cout, cin = w.shape[:2]
    sw = torch.zeros((2, 2, 2, cout, cin, 2, 2, 2), dtype=w.dtype)
    for pz in range(2):
        for py in range(2):
            for px in range(2):
                for ez in range(2):
                    for ey in range(2):
                        for ex in range(2):
                            for dz in GROUPS[pz, ez]:
                                for dy in GROUPS[py, ey]:
                                    for dx in GROUPS[px, ex]:
                                        sw[pz, py, px, :, :, ez, ey, ex] += w[:, :, dz, dy, dx]
    return sw


def subpixel_upconv(x, w, out_size=None):
    """x (c_in, D, H, W) stored tensor -> (c_out, 2D, 2H, 2W), cropped to out_size"""
    cin, D, H, W = x.shape
    sw = subpixel_weights(w)
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))[None]                    # zero padding of the stored tensor
    out = torch.zeros((w.shape[0], 2 * D, 2 * H, 2 * W), dtype=x.dtype)
    for pz in range(2):
        for py in range(2):
            for px in range(2):
                y = F.conv3d(xp, sw[pz, py, px])[0]             # y[j] = sum_e w[e] stored[j - 1 + e]; output 2i + p reads j = i + p
                out[:, pz::2, py::2, px::2] = y[:, pz:pz + D, py:py + H, px:px + W]
    if out_size is not None:
        out = out[:, :out_size[0], :out_size[1], :out_size[2]]
    return out


@pytest.mark.parametrize("dims,crop", [((1, 1, 1), None), ((2, 2, 2), None), ((7, 7, 7), None), ((1, 2, 7), None), ((7, 1, 2), None),
                                       ((4, 5, 6), None), ((5, 5, 5), (9, 9, 9)), ((7, 7, 7), (13, 13, 13)), ((2, 7, 1), (3, 14, 1)),
                                       ((3, 4, 5), (5, 8, 9))])
def test_upsampled_conv_equals_eight_parity_convs(dims, crop):
    g = torch.Generator().manual_seed(sum(dims) * 7 + (sum(crop) if crop else 0))
    cin, cout = 5, 4
    x = torch.randn((cin,) + dims, generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g, dtype=torch.float64)
    ref = F.conv3d(F.interpolate(x[None], scale_factor=2, mode="nearest"), w, padding=1)[0]
    if crop is not None:
        ref = ref[:, :crop[0], :crop[1], :crop[2]]
    got = subpixel_upconv(x, w, crop)
    assert got.shape == ref.shape
    err = float((got - ref).norm() / ref.norm())
    print(f"dims {dims} crop {crop}: rel {err:.2e}")
    assert err < 1e-12, err


def test_summed_groups_never_straddle_the_border():
    """Every group of original taps that is summed reads ONE stored voxel, so it lies wholly inside or wholly outside the
    stored tensor and zero padding stays exact: floor((2i + p + d) / 2) is the same for all d of a group."""
    for (p, e), taps in GROUPS.items():
        for i in range(-1, 9):
            assert {(2 * i + p + d - 1) // 2 for d in taps} == {i - 1 + p + e}
    assert sorted(t for (p, e), ts in GROUPS.items() if p == 0 for t in ts) == [0, 1, 2]
    assert sorted(t for (p, e), ts in GROUPS.items() if p == 1 for t in ts) == [0, 1, 2]
