"""pixie_unet_forward_pair against pixie_unet_forward: two seeded networks over one input, once through the pair call (both plans
walked into launch lists, the levels below full resolution zipped and grouped: csrc/launch_list.h, csrc/unet_exec.hip) and once
each through their own pass.  The pair call only changes which launch carries a workgroup's work, so the outputs must be EQUAL
(torch.equal), for networks that group everything the twins cover, for odd grids, with attention, for pairs that match only in
part or not at all, on a reused workspace, with grouping switched off (the merged order alone), and through predict_material_field
with the pair route on and off."""
import ctypes as C

import pytest
import torch

from pixie_amd.synthetic import feature_grid
from pixie_amd.unet_plan import synthetic_state_dict

pytestmark = pytest.mark.gpu

# the small cube of the issue: the inner levels (8^3, 4^3, 2^3) hold split-K convs with their reduce, the folded skip, the sub-pixel
# up-conv and both finalise modes
SMALL = dict(feature_channels=16, cond_dim=32, model_channels=32, num_res_blocks=1, channel_mult=(1, 1, 2, 4), attention_resolutions=(), grid_size=16)


def network(kind, kw, seed, device, precision="f16x3"):
    from pixie_amd.unet import RegressionUNet, SegmentationUNet
    net = SegmentationUNet(num_classes=8, **kw) if kind == "seg" else RegressionUNet(out_channels=3, **kw)
    net.load_numpy_state(synthetic_state_dict(net.cfg, seed))
    net = net.to(device).eval()
    net.conv_precision = precision
    net._prepare(device)
    return net


def pair_forward(n0, n1, x, buffers=None):
    """-> (out0, out1, (launches of the two single passes, launches issued, grouped launches, grouped convolutions)); buffers: (ws0, ws1) to reuse"""
    from pixie_amd import _lib
    lib = _lib.load()
    D = int(x.shape[1])
    outs = [torch.full((n.cfg.out_channels, D, D, D), float("nan"), device=x.device) for n in (n0, n1)]
    nbytes = [n._handle.workspace_bytes(D, D, D) for n in (n0, n1)]
    wss = buffers or [torch.full((nb,), 255, dtype=torch.uint8, device=x.device) for nb in nbytes]
    counts = (C.c_int32 * 4)()
    _lib.check(lib.pixie_unet_forward_pair(n0._handle._h, n1._handle._h, x.data_ptr(), D, D, D, outs[0].data_ptr(), outs[1].data_ptr(),
                                           wss[0].data_ptr(), nbytes[0], wss[1].data_ptr(), nbytes[1], _lib.current_stream_ptr(), counts),
               "pixie_unet_forward_pair")
    return outs[0], outs[1], tuple(counts)


def check_pair(n0, n1, x, what):
    want = [n._handle.forward(x) for n in (n0, n1)]
    o0, o1, counts = pair_forward(n0, n1, x)
    print(f"{what}: {counts[0]} launches as two passes, {counts[1]} in the pair call, {counts[2]} of them grouped ({counts[3]} convolutions)")
    assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1]).all())
    assert float(want[0].abs().max()) > 0 and float(want[1].abs().max()) > 0          # seeded heads: not the zero-initialised ones
    assert torch.equal(o0, want[0]), f"{what}: network 0 differs from its own pass"
    assert torch.equal(o1, want[1]), f"{what}: network 1 differs from its own pass"
    assert counts[1] == counts[0] - counts[2]      # a grouped launch stands for two, nothing else is added or lost
    return counts


@pytest.mark.parametrize("group", ["grouped", "zipped_only"])
@pytest.mark.parametrize("D", [16, 12], ids=["cube16", "odd12"])      # 12 -> 6 -> 3 -> 2: the up-convs crop (4 -> 3), partial tiles
def test_pair_equals_two_passes(hip_device, monkeypatch, D, group):
    if group == "zipped_only":
        monkeypatch.setenv("PIXIE_UNET_PAIR_GROUP", "0")
    kw = dict(SMALL, grid_size=D)
    seg, cont = network("seg", kw, 11, hip_device), network("cont", kw, 12, hip_device)
    x = torch.from_numpy(feature_grid(D, kw["feature_channels"], seed=5)).to(hip_device)[0].contiguous()
    counts = check_pair(seg, cont, x, f"{D}^3 {group}")
    if group == "zipped_only":
        assert counts[2] == 0


# model_channels 64, as shipped, on a grid large enough that the levels below full resolution launch conv instantiations of the
# grouping table (csrc/conv3d_f16x3.hip: conv16_group_kernel).  Asked of the planner for these shapes: at 64^3 with channel_mult
# (1, 2, 4) the 32^3 level runs <3,2,4> in 4 split-K slices (grid 64 x 2 x 4, the most frequent inner launch of the 128^3 scene), the
# 16^3 level <1,2,x> and the sub-pixel <2> up-conv.  (The 128^3 scene itself goes through predict_material_field, and so through the
# pair route, in tests/test_unet_hip.py.)
SHIPPED_WIDTH = dict(SMALL, model_channels=64, channel_mult=(1, 2, 4), grid_size=64)


def test_pair_at_the_shipped_width(hip_device):
    seg, cont = network("seg", SHIPPED_WIDTH, 61, hip_device), network("cont", SHIPPED_WIDTH, 62, hip_device)
    x = torch.from_numpy(feature_grid(64, SHIPPED_WIDTH["feature_channels"], seed=2)).to(hip_device)[0].contiguous()
    check_pair(seg, cont, x, "64^3, model_channels 64")


def test_the_grouped_path_is_taken(hip_device):
    """The equality cases of this file hold whether or not a kernel has a grouped twin (a launch without one goes out as two).  This
    case alone states that the twins this tree has ARE used, so that the others do exercise them: below full resolution two
    networks of one architecture group the reduces and the finalisers (dozens), and at the shipped width convolutions of the
    grouping table.  It is the one case to revisit when a twin is taken out."""
    for kw, least_grouped, least_convs in ((SMALL, 20, 0), (SHIPPED_WIDTH, 20, 4)):
        seg, cont = network("seg", kw, 71, hip_device), network("cont", kw, 72, hip_device)
        D = kw["grid_size"]
        x = torch.from_numpy(feature_grid(D, kw["feature_channels"], seed=1)).to(hip_device)[0].contiguous()
        _, _, counts = pair_forward(seg, cont, x)
        print(f"{D}^3, model_channels {kw['model_channels']}: {counts}")
        assert counts[1] == counts[0] - counts[2]
        assert counts[2] >= least_grouped, "the reduces and finalisers below full resolution did not go out grouped"
        assert counts[3] >= least_convs, "no convolution below full resolution went out grouped"


def test_pair_with_attention_levels(hip_device):
    kw = dict(SMALL, attention_resolutions=(2, 4))
    seg, cont = network("seg", kw, 21, hip_device), network("cont", kw, 22, hip_device)
    x = torch.from_numpy(feature_grid(16, kw["feature_channels"], seed=6)).to(hip_device)[0].contiguous()
    check_pair(seg, cont, x, "attention at 8^3 and 4^3")


def test_mismatched_pairs_group_less_and_stay_equal(hip_device):
    x = torch.from_numpy(feature_grid(16, SMALL["feature_channels"], seed=7)).to(hip_device)[0].contiguous()
    seg = network("seg", SMALL, 31, hip_device)
    wide = network("cont", dict(SMALL, model_channels=64), 32, hip_device)
    full = check_pair(seg, network("cont", SMALL, 33, hip_device), x, "matching pair")
    part = check_pair(seg, wide, x, "model_channels 32 and 64")
    assert part[2] <= full[2] and (part[2] < full[2] or full[2] == 0)
    exact = network("cont", SMALL, 33, hip_device, precision="f32")
    part = check_pair(seg, exact, x, "f16x3 and exact fp32")
    assert part[2] <= full[2] and (part[2] < full[2] or full[2] == 0)
    part = check_pair(exact, seg, x, "exact fp32 and f16x3")       # the first network computes no input statistics to share
    assert part[2] <= full[2] and (part[2] < full[2] or full[2] == 0)
    deeper = network("cont", dict(SMALL, num_res_blocks=2), 34, hip_device)
    check_pair(seg, deeper, x, "1 and 2 residual blocks per level")      # lists of different length


def test_repeat_calls_on_the_same_buffers(hip_device):
    """What one pair call leaves in the workspaces (statistics, |x|max slots, split-K slices) is the next one's garbage: the head of
    each workspace is cleared by the pass itself, and a second input through the same buffers gives that input's result."""
    seg, cont = network("seg", SMALL, 41, hip_device), network("cont", SMALL, 42, hip_device)
    xs = [torch.from_numpy(feature_grid(16, SMALL["feature_channels"], seed=s)).to(hip_device)[0].contiguous() for s in (8, 9)]
    nbytes = [n._handle.workspace_bytes(16, 16, 16) for n in (seg, cont)]
    wss = [torch.full((nb + 4096,), 255, dtype=torch.uint8, device=hip_device) for nb in nbytes]
    x = torch.empty_like(xs[0])
    for i in (0, 1, 1, 0):
        x.copy_(xs[i])
        want = [n._handle.forward(x) for n in (seg, cont)]
        o0, o1, _ = pair_forward(seg, cont, x, buffers=wss)
        assert torch.equal(o0, want[0]) and torch.equal(o1, want[1]), f"call with input {i}"
        assert all(bool((ws[nb:] == 255).all()) for ws, nb in zip(wss, nbytes))      # and it stays inside what each network asked for


def test_pair_call_rejects_bad_arguments(hip_device):
    from pixie_amd import _lib
    lib = _lib.load()
    seg, cont = network("seg", SMALL, 41, hip_device), network("cont", SMALL, 42, hip_device)
    x = torch.zeros((16, 16, 16, 16), device=hip_device)
    out = [torch.empty((8, 16, 16, 16), device=hip_device), torch.empty((3, 16, 16, 16), device=hip_device)]
    nb = [n._handle.workspace_bytes(16, 16, 16) for n in (seg, cont)]
    ws = [torch.empty(n, dtype=torch.uint8, device=hip_device) for n in nb]

    def call(h0, h1, w0, w1, b1, d=16):
        return lib.pixie_unet_forward_pair(h0, h1, x.data_ptr(), d, d, d, out[0].data_ptr(), out[1].data_ptr(), w0.data_ptr(), nb[0], w1.data_ptr(), b1,
                                           _lib.current_stream_ptr(), None)
    assert call(seg._handle._h, seg._handle._h, ws[0], ws[1], nb[1]) != 0          # one handle twice
    assert call(seg._handle._h, cont._handle._h, ws[0], ws[0], nb[1]) != 0         # one workspace for both
    assert call(seg._handle._h, cont._handle._h, ws[0], ws[1], nb[1] - 256) != 0 and b"workspace" in lib.pixie_last_error()
    assert call(seg._handle._h, cont._handle._h, ws[0], ws[1], nb[1], d=8) != 0    # not the networks' grid
    assert call(seg._handle._h, cont._handle._h, ws[0], ws[1], nb[1]) == 0


def test_predict_material_field_pair_route_on_and_off(hip_device, monkeypatch):
    """The pair route (one captured graph of the pair call) and the two networks' own graphs give the same four arrays, on the eager
    first call, the capturing second and the replays; a new input in the same buffer is followed."""
    from pixie_amd.unet import predict_material_field
    monkeypatch.delenv("PIXIE_DUAL_STREAM", raising=False)
    seg, cont = network("seg", SMALL, 51, hip_device), network("cont", SMALL, 52, hip_device)
    assert seg.use_graph and cont.use_graph and seg.executor == "c"
    feats = [torch.from_numpy(feature_grid(16, SMALL["feature_channels"], seed=s)).to(hip_device) for s in (3, 4)]
    x = torch.empty_like(feats[0])
    order = (0, 0, 0, 1, 0)
    results = {}
    for route in ("1", "0"):
        monkeypatch.setenv("PIXIE_UNET_PAIR", route)
        results[route] = []
        for i in order:
            x.copy_(feats[i])
            results[route].append([t.clone() for t in predict_material_field(seg, cont, x, dual_stream=False)])
    graphs = seg.__dict__.get("_pair_graphs", {})
    assert x.data_ptr() in graphs and not graphs.get("failed"), "the pair route was not taken, or its capture failed"
    for k, i in enumerate(order):
        for a, b, name in zip(results["1"][k], results["0"][k], ("combined", "seg_pred", "seg_logits", "cont_pred")):
            assert a.shape == b.shape and torch.equal(a, b), f"call {k} (input {i}): {name} differs between the routes"
    assert not torch.equal(results["1"][2][3], results["1"][3][3])      # the two inputs do give different fields
