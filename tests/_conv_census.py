"""Which convolution launches does the product issue, and which do the operator tests issue?  TEST INFRASTRUCTURE ONLY.

A launch's CLASS is what decides which code of csrc/conv3d_f16x3.hip runs: the path, the kernel instantiation <KS, MB, NB>, split-K
or not, stride, the upsampling form, one or two inputs, the prologue, residual, folded skip, epilogue statistics, odd crop, per axis
the number of tiles (1, 2, more) and whether the last one is ragged, and whether the launch reserves the transposing epilogue's
LDS.  Variant, split factor and tile geometry are READ FROM THE LIBRARY (pixie_conv_kernel_variant / pixie_conv_tile_geometry
of the PIXIE_DIAG build: pure host functions of the descriptor, no device needed); the descriptor is the one
pixie_amd.unet.fill_conv_desc builds for HipOps.conv.  Nothing of the tile heuristic is restated here.

A split-K launch never hands d_out_stats to the conv kernel (conv3d_f16x3_forward clears it: the slices are raw partial outputs),
so LaunchClass.stats of a split launch is False whatever was asked for.  What was asked for decides the code of the REDUCE behind
it, and that is the launch's ReduceClass: statistics or not (splitk_reduce_stats_kernel / splitk_reduce_kernel), the vector or the
scalar form (osp % 4; torch tensors are 16-byte aligned), the segments per channel (1, 2-256, more), whether the last segment is
ragged, residual, and the slices (2, more).  Segment count and length are READ FROM THE LIBRARY too (pixie_conv_stats_layout, the
PIXIE_DIAG export of the StatParts the finalise kernels read).

A FinaliseClass is the class of one pixie_stats_finalize ("sums") or pixie_stats_norm_finalize ("layernorm" / "groupnorm")
launch: per part what the producer left behind -- final sums, float32 tile partials (at most 256 per channel or more: the
`t += 256` loop of block_channel_sums; c_out padded or not: tstride), float64 segment partials (same buckets) -- and for a
GroupNorm over two parts whether a group straddles the boundary c0.

`product_walk` walks a network's plan with RecordingOps, a stand-in for HipOps that allocates nothing (shape-only `meta`
tensors) and records every conv launch's class, every reduce's and every finalise's; it takes the route HipOps takes
(tests/test_conv_variant_census.py::test_the_stand_in_takes_the_product_route holds the two together).  `operator_class` /
`operator_reduce_class` / `finalise_class` give the classes of one operator-test case."""
import ctypes as C
from collections import namedtuple

import torch

from pixie_amd import _lib
from pixie_amd.unet import ACT_NONE, HipOps, PendingStats, UNetRunner, fill_conv_desc
from pixie_amd.unet_plan import UNetConfig, is_norm_key, param_shapes

LaunchClass = namedtuple("LaunchClass", "path ks mb nb split stride up two_inputs prologue residual fold stats crop x y z epi_lds")
ReduceClass = namedtuple("ReduceClass", "stats form segments ragged residual slices")
FinaliseClass = namedtuple("FinaliseClass", "mode parts straddle")
FINAL = ("final",)
GEOMETRY_FIELDS = ("TX", "TY", "TZ", "tiles_x", "tiles_y", "tiles_z", "epi_lds", "slices", "MB", "NB")


def _meta(shape, dtype=torch.float32):
    return torch.empty(tuple(int(v) for v in shape), dtype=dtype, device="meta")


def _stand_in_addr(t):
    return 1 if t is not None else None     # "present"; nothing dereferences it


def tile_geometry(desc):
    """dict of GEOMETRY_FIELDS for a descriptor, or None if it takes neither tiled launch (first-generation exact kernel)"""
    out = (C.c_int32 * 10)()
    if _lib.load(diag=True).pixie_conv_tile_geometry(C.byref(desc), out) != 0:
        return None
    return dict(zip(GEOMETRY_FIELDS, (int(v) for v in out)))


def stats_layout(desc):
    """dict(n, cstride, tstride, f64, segment, coutp): where the launch of `desc` leaves its partial statistics (None: no f16x3 launch)"""
    out = (C.c_int64 * 6)()
    if _lib.load(diag=True).pixie_conv_stats_layout(C.byref(desc), out) != 0:
        return None
    return dict(zip(("n", "cstride", "tstride", "f64", "segment", "coutp"), (int(v) for v in out)))


def _many(n):
    return ">256" if n > 256 else "<=256"


def reduce_class(desc, out_shape):
    """ReduceClass of a filled descriptor (None: the launch does not split)"""
    g = tile_geometry(desc)
    if g is None or g["slices"] <= 1:
        return None
    residual, slices = bool(desc.d_residual), "2" if g["slices"] == 2 else ">2"
    if not desc.d_out_stats:       # splitk_reduce_kernel: one thread per element, no form, no segments
        return ReduceClass(False, "-", "-", False, residual, slices)
    lay = stats_layout(desc)
    osp = int(out_shape[1]) * int(out_shape[2]) * int(out_shape[3])
    assert lay["f64"] and lay["segment"] > 0 and lay["n"] == -(-osp // lay["segment"]), (lay, osp)
    return ReduceClass(True, "vector" if osp % 4 == 0 else "scalar", "1" if lay["n"] == 1 else ("2-256" if lay["n"] <= 256 else ">256"),
                       osp % lay["segment"] != 0, residual, slices)


def part_kind(desc):
    """what a launch with statistics leaves behind for the finalise: ("tile", count bucket, c_out padded?) / ("segment", count bucket)"""
    lay = stats_layout(desc)
    if lay["f64"]:
        return ("segment", _many(lay["n"]))
    return ("tile", _many(lay["n"]), lay["coutp"] != desc.c_out)


def finalise_class(mode, parts, groups=1):
    """FinaliseClass of one finalise launch.  mode: "sums" (pixie_stats_finalize), 0 / 1 (pixie_stats_norm_finalize: LayerNorm /
    GroupNorm); parts: [(channels, pixie_conv_desc of the producer, or None where the part's sums are final)]"""
    kinds = tuple(FINAL if d is None else part_kind(d) for _, d in parts)
    straddle = False
    if mode == 1 and len(parts) == 2:
        straddle = parts[0][0] % ((parts[0][0] + parts[1][0]) // groups) != 0
    return FinaliseClass({"sums": "sums", 0: "layernorm", 1: "groupnorm"}[mode], kinds, straddle)


def classify(desc, out_shape):
    """LaunchClass of a filled descriptor (None: not a tiled launch)"""
    g = tile_geometry(desc)
    if g is None:
        return None
    f16 = bool(desc.d_w16)
    sub = False
    if f16:
        sl = C.c_int(1)
        v = int(_lib.load(diag=True).pixie_conv_kernel_variant(C.byref(desc), C.byref(sl)))
        assert int(sl.value) == g["slices"], (v, sl.value, g)
        sub = 8300 <= v < 8400
        assert sub or v == 9324 or v == desc.ksize * 100 + g["MB"] * 10 + g["NB"], (v, g)
    od, oh, ow = (int(v) for v in out_shape[1:])
    up = 2 if desc.upsample else 1
    pad = 1 if desc.ksize == 3 else 0
    natural = tuple((n * up + 2 * pad - desc.ksize) // desc.stride + 1 for n in (desc.in_d, desc.in_h, desc.in_w))
    ext = tuple((n + 1) // 2 for n in (od, oh, ow)) if sub else (od, oh, ow)     # sub-pixel tiles lie over the stored voxels

    def axis(n_tiles, extent, t):
        return (min(n_tiles, 3), extent % t != 0)

    return LaunchClass(
        path="f16x3" if f16 else "f32", ks=int(desc.ksize), mb=g["MB"], nb=g["NB"], split=g["slices"] > 1, stride=int(desc.stride),
        up="none" if not desc.upsample else ("sub-pixel" if sub else "27-tap"), two_inputs=desc.c1 > 0,
        prologue="none" if not desc.d_pro_a else ("channel+spatial" if desc.d_gamma else "channel"),
        residual=bool(desc.d_residual), fold=bool(desc.d_skip_w16), stats=bool(desc.d_out_stats) and g["slices"] == 1, crop=(od, oh, ow) != natural,
        x=axis(g["tiles_x"], ext[2], g["TX"]), y=axis(g["tiles_y"], ext[1], g["TY"]), z=axis(g["tiles_z"], ext[0], g["TZ"]),
        epi_lds=bool(g["epi_lds"]))


def describe(desc, out_shape):
    """(LaunchClass, geometry dict) of a descriptor"""
    return classify(desc, out_shape), tile_geometry(desc)


def operator_desc(precision, cins, cout, dims, ksize, *, stride=1, upsample=False, prologue="none", residual=False, stats=False,
                  out_size=None, skip_cins=None, subpixel=False, split_k=True, split_stats=False):
    """The descriptor HipOps.conv builds for an operator-test case given by shapes alone -> (desc, output shape).  `split_stats`:
    the call passes defer_stats (and leaves split_stats on), so a split-K launch takes the statistics in its reduce."""
    lib = _lib.load()
    parts = [_meta((c,) + tuple(dims)) for c in cins]
    cin = sum(cins)
    one = _meta((1,))
    kw = dict(stride=stride, upsample=upsample, residual=one if residual else None, out_size=out_size, split_k=split_k)
    if prologue != "none":
        kw["pro"] = (_meta((cin,)), _meta((cin,)))
    if prologue == "channel+spatial":
        kw["affine"] = (_meta(dims), _meta(dims))
    if precision == "f16x3":
        kw.update(w16=one, subpixel=subpixel, out_amax=one if stats else None)
        if prologue == "none":
            kw["in_amax"] = [one] * len(cins)
        else:
            kw["in_bound"] = 1.0
        if skip_cins:
            kw["skip"] = dict(parts=[_meta((c,) + tuple(dims)) for c in skip_cins], w16=one, bias=one, amax=[one] * len(skip_cins))
        packed = None
    else:
        assert not subpixel and not skip_cins and not stats
        packed = one
    desc, out, _, _ = fill_conv_desc(lib, _meta, parts, packed, one, cout, ksize, addr=_stand_in_addr, split_stats=split_stats, **kw)
    return desc, tuple(out.shape)


def operator_class(*args, **kw):
    return classify(*operator_desc(*args, **kw))


def operator_reduce_class(*args, **kw):
    return reduce_class(*operator_desc(*args, **kw))


class RecordingOps:
    """The operators UNetRunner needs, launching nothing: convolutions build the descriptor HipOps.conv would build and record
    its class (and its reduce's), the finalises record theirs; every tensor is shape-only."""

    def __init__(self, split_k=True):
        self.lib = _lib.load()
        self.split_k = split_k
        self.device = torch.device("meta")
        self.records = []           # (layer key, LaunchClass or None, output shape)
        self.reduces = []           # (layer key, ReduceClass, output shape) of the split launches among them
        self.finalises = []         # (the convolution launched last, FinaliseClass)
        self.layer = "?"

    pack_conv = pack_conv16 = pack_conv_subpixel = staticmethod(lambda weight: _meta((1,)))
    f16x3_ok = staticmethod(HipOps.f16x3_ok)
    skip_foldable = HipOps.skip_foldable

    def conv(self, parts, packed_w, bias, cout, ksize, stride=1, upsample=False, pro=None, affine=None, act=ACT_NONE, residual=None,
             w16=None, in_amax=None, in_bound=0.0, out_amax=None, out_size=None, skip=None, subpixel=False, defer_stats=False,
             split_stats=True):
        desc, out, stats, _ = fill_conv_desc(self.lib, _meta, parts, packed_w, bias, cout, ksize, stride=stride, upsample=upsample,
                                             pro=pro, affine=affine, act=act, residual=residual, w16=w16, in_amax=in_amax,
                                             in_bound=in_bound, out_amax=out_amax, out_size=out_size, skip=skip, subpixel=subpixel,
                                             split_k=self.split_k, split_stats=defer_stats and split_stats, addr=_stand_in_addr)
        self.records.append((self.layer, classify(desc, out.shape), tuple(out.shape)))
        red = reduce_class(desc, out.shape)
        if red is not None:
            self.reduces.append((self.layer, red, tuple(out.shape)))
        sums = None
        if desc.d_out_stats:       # as HipOps.conv
            sums = PendingStats(stats, desc, cout)
            if not defer_stats:
                sums = self.stats_finalize(sums)
        if out_amax is not None:
            return out, sums
        return out

    def stats_finalize(self, pending):
        self.finalises.append((self.layer, finalise_class("sums", [(pending.cout, pending.desc)])))
        return _meta((pending.cout, 2), torch.float64)

    def stats_norm_finalize(self, parts, spatial, mode, groups=1, eps=1e-5, weight=None, bias=None):
        pend = [isinstance(p, PendingStats) for p in parts]
        given = [(p.cout, p.desc) if is_p else (int(p.shape[0]), None) for p, is_p in zip(parts, pend)]
        self.finalises.append((self.layer, finalise_class(mode, given, groups)))
        sums = [_meta((c, 2), torch.float64) if is_p else p for (c, _), p, is_p in zip(given, parts, pend)]
        c = sum(c for c, _ in given)
        return _meta((c,)), _meta((c,)), sums

    def channel_sums(self, x):
        return _meta((x.shape[0], 2), torch.float64)

    def channel_stats(self, x, amax_slot):
        return _meta((x.shape[0], 2), torch.float64)

    def norm_finalize(self, sums, spatial, mode, groups=1, eps=1e-5, weight=None, bias=None):
        return _meta((sums.shape[0],)), _meta((sums.shape[0],))

    def attention(self, qkv, channels, tokens):
        return _meta((channels, tokens))


class _Walk(UNetRunner):
    def _conv(self, cache, parts, wkey, *a, **kw):
        self.ops.layer = wkey
        return super()._conv(cache, parts, wkey, *a, **kw)

    def _absmax(self, key):     # the magnitude bound's value does not choose a kernel
        return 1.0, 0.0


def product_walk(cfg: UNetConfig, precision: str, subpixel: bool, dims=None):
    """The RecordingOps after one forward pass of `cfg`, as UNetRunner + HipOps launch it (the C executor walks the same plan
    and fills the same descriptors; tests/test_unet_hip.py holds the two bit-identical): .records, .reduces, .finalises"""
    params = {k: _meta(s) for k, s in param_shapes(cfg).items()}
    ops = RecordingOps()
    run = _Walk(cfg, params, ops, precision=precision)
    run.fuse_stats = run.fold_skip = run.split_stats = True
    run.subpixel = subpixel
    d = cfg.grid_size
    run.forward(_meta((cfg.feature_channels,) + (tuple(dims) if dims else (d, d, d))))
    return ops


def product_launches(cfg: UNetConfig, precision: str, subpixel: bool, dims=None):
    """[(layer key, LaunchClass, output shape)] of that pass"""
    return product_walk(cfg, precision, subpixel, dims).records
