"""Census of convolution launch classes (CPU only, nothing is launched): every class the product's networks issue has an
operator test, and every one of the twelve kernel instantiations has one -- unsplit on both paths, split on the f16x3 path.

The class of a launch (tests/_conv_census.py) is read from the library's own selection code through pixie_conv_kernel_variant and
pixie_conv_tile_geometry on the descriptor pixie_amd.unet.fill_conv_desc builds, for the product (the plan of every claimed
configuration, walked with a recording stand-in for HipOps) and for the operator tests (their case tables).  A change of the
tile heuristic or of a network plan that opens a gap fails here, naming the layer; so does deleting a row of
tests/test_conv_variants_hip.VARIANT_CASES that a product class depends on.

The same for what follows a convolution: every class of split-K reduce (ReduceClass) and of finalise launch (FinaliseClass)
the networks issue has a row in tests/test_splitk_reduce_stats_hip.py, and both forms of the reduce have rows with one segment,
with several and with a ragged last one.  The walk takes the product's route only while the stand-in offers what HipOps
offers: test_the_stand_in_takes_the_product_route holds the two together, from the probes UNetRunner itself makes."""
import inspect
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_census as cc                      # noqa: E402
import test_conv_subpixel_hip as tsub          # noqa: E402
import test_splitk_reduce_stats_hip as trs     # noqa: E402
import test_conv_variants_hip as tvar          # noqa: E402
import test_unet_hip as tu                     # noqa: E402
import pixie_amd.unet as unet_module           # noqa: E402
from pixie_amd.unet import HipOps              # noqa: E402
from pixie_amd.unet_plan import UNetConfig     # noqa: E402

# the configurations the project claims (bench.py, tests/golden): both heads where the head changes a launch
PRODUCT = {
    "baseline2_128_seg": UNetConfig(64, 32, 64, 3, (1, 1, 2, 4), (), 128, 8),
    "baseline2_128_cont": UNetConfig(64, 32, 64, 3, (1, 1, 2, 4), (), 128, 3),
    "shipped_64x768": UNetConfig(768, 32, 64, 3, (1, 1, 2, 4), (), 64, 3),
    "config4_256x128": UNetConfig(128, 32, 64, 3, (1, 1, 2, 4), (), 256, 8),
    "golden_odd9": UNetConfig(32, 32, 32, 1, (1, 2), (), 9, 8),
    "golden_odd13": UNetConfig(64, 32, 32, 1, (1, 2, 2), (), 13, 8),
}
INSTANTIATIONS = [(ks, mb, nb) for ks in (3, 1) for mb in (2, 1) for nb in (4, 2, 1)]
# instantiations that no legal descriptor reaches split, by name with the reason.  None: <KS,1,NB> splits whenever c_out <= 32 has
# too few tiles for the chip and c_in >= 64 leaves chunks to split (rows k3-256to32-split, k3-64to32-split, pw256to32-split, pw64to32).
UNREACHABLE_SPLIT = {}


def operator_launches(without_rows=()):
    """{LaunchClass: [operator case id]} of every HipOps.conv call the operator tests' case tables make"""
    out = {}

    def add(cid, precision, cins, cout, dims, k, **kw):
        if precision == "f16x3" and not HipOps.f16x3_ok([cc._meta((c, 1)) for c in cins], kw.get("stride", 1)):
            return
        cls = cc.operator_class(precision, cins, cout, dims, k, **kw)
        if cls is not None:
            out.setdefault(cls, []).append(cid)

    # test_unet_hip.test_conv3d_operator
    for i, (cins, cout, dims, k, stride, ups, prologue, act, res) in enumerate(tu.CONV_CASES):
        pro = "none" if not prologue else ("channel" if ups else "channel+spatial")
        for prec in ("f32", "f16x3"):
            add(f"test_conv3d_operator[c{i}-{prec}]", prec, cins, cout, dims, k, stride=stride, upsample=ups, prologue=pro, residual=res)
    # test_conv3d_epilogue_statistics (split-K off), test_conv3d_split_k (split, split with statistics asked for, unsplit)
    for cins, cout, dims, k in tu.STATS_SHAPES:
        add(f"test_conv3d_epilogue_statistics[{cins}-{cout}-{dims}]", "f16x3", cins, cout, dims, k, stats=True, split_k=False)
    for cins, cout, dims, k in tu.SPLIT_K_SHAPES:
        for stats, sk in ((True, True), (False, True), (False, False)):
            add(f"test_conv3d_split_k[{cins}-{cout}-{dims}]", "f16x3", cins, cout, dims, k, residual=True, stats=stats, split_k=sk)
    # test_conv3d_folded_skip_convolution: the fold with and without statistics, the skip convolution alone, the two-launch route
    for cin, skip_c, cout, dims, res, sk in tu.FOLD_SHAPES:
        cid = f"test_conv3d_folded_skip_convolution[{cin}-{skip_c}-{cout}-{dims}]"
        for stats in (True, False):
            add(cid, "f16x3", (cin,), cout, dims, 3, prologue="channel+spatial", residual=res, skip_cins=skip_c, stats=stats, split_k=sk)
        add(cid, "f16x3", skip_c, cout, dims, 1, split_k=sk)
        add(cid, "f16x3", (cin,), cout, dims, 3, prologue="channel+spatial", residual=True, split_k=sk)
    # test_conv_subpixel_hip: operator, statistics (split-K off), split-K, and the 27-tap form of case 1
    spro = lambda prologue: "none" if not prologue else ("channel+spatial" if prologue == "ln" else "channel")
    for i, (cins, cout, dims, prologue, act, res, osz) in enumerate(tsub.SUBPIXEL_CASES):
        add(f"test_subpixel_upconv_operator[s{i}]", "f16x3", cins, cout, dims, 3, upsample=True, subpixel=True, prologue=spro(prologue),
            residual=res, out_size=osz)
        if i in tsub.STATS_CASES:
            add(f"test_subpixel_upconv_epilogue_statistics[s{i}]", "f16x3", cins, cout, dims, 3, upsample=True, subpixel=True,
                prologue=spro(prologue), residual=res, out_size=osz, stats=True, split_k=False)
    for cins, cout, dims in tsub.SUBPIXEL_SPLIT_K_SHAPES:
        for stats, sk in ((True, True), (False, True), (False, False)):
            add(f"test_subpixel_upconv_split_k[{cins}-{cout}-{dims}]", "f16x3", cins, cout, dims, 3, upsample=True, subpixel=True,
                residual=True, stats=stats, split_k=sk)
    cins, cout, dims, prologue, act, res, osz = tsub.SUBPIXEL_CASES[1]
    add("test_subpixel_agrees_with_the_27_tap_form", "f16x3", cins, cout, dims, 3, upsample=True, prologue=spro(prologue), residual=res)
    for case in tvar.VARIANT_CASES:
        if case.id not in without_rows:
            for prec in tvar.runs(case):
                for sk, stats in tvar.launches(case, prec):
                    add(f"test_conv_variant[{case.id}-{prec}]", prec, case.cins, case.cout, case.dims, case.k, stride=case.stride,
                        upsample=case.up != "none", subpixel=case.up == "sub-pixel", prologue=case.pro, residual=case.res,
                        out_size=case.out_size, skip_cins=case.skip if prec == "f16x3" else None, stats=stats, split_k=sk)
    # (tests/test_splitk_reduce_stats_hip.py launches convolutions too, but compares none with a float64 convolution: its rows
    # count for the reduce and the finalise classes below, not here)
    return out


def _producer_kw(prod, split_k, stats):
    """operator_desc arguments of a HipOps.conv call of tests/test_splitk_reduce_stats_hip.py (its Producer)"""
    return dict(cins=prod.cins, cout=prod.cout, dims=prod.dims, ksize=prod.k, upsample=prod.sub, subpixel=prod.sub, residual=prod.res,
                out_size=prod.out_size, stats=stats, split_k=split_k, split_stats=stats)


def operator_reduces(without_rows=()):
    """{ReduceClass: [operator case id]} of the rows of test_splitk_reduce_stats_hip.REDUCE_ROWS; every row must split"""
    out = {}
    for rid, prod in trs.REDUCE_ROWS:
        if rid in without_rows:
            continue
        for sk, stats in trs.reduce_row_launches(prod):
            cls = cc.operator_reduce_class("f16x3", **_producer_kw(prod, sk, stats))
            assert cls is not None, f"{rid}: this row does not split"
            out.setdefault(cls, []).append(f"test_splitk_reduce_statistics[{rid}]")
    return out


def operator_finalises(without_rows=()):
    """{FinaliseClass: [operator case id]} of the pixie_stats_norm_finalize calls of test_splitk_reduce_stats_hip, and (mode
    "sums") of the pixie_stats_finalize calls that are checked against float64 there: every reduce row's, the tile producer's"""
    out = {}
    for rid, prod in trs.REDUCE_ROWS:
        if rid not in without_rows:
            desc, _ = cc.operator_desc("f16x3", **_producer_kw(prod, prod.split_k, True))
            out.setdefault(cc.finalise_class("sums", [(prod.cout, desc)]), []).append(f"test_splitk_reduce_statistics[{rid}]")
    if "tile-partials" not in without_rows:
        desc, _ = cc.operator_desc("f16x3", **_producer_kw(trs.TILE_PRODUCER, False, True))
        out.setdefault(cc.finalise_class("sums", [(trs.TILE_PRODUCER.cout, desc)]), []).append("test_merged_finalise_of_tile_partials")

    def part(p):
        if isinstance(p, trs.Final):
            return (p.prod.cout, None), _producer_shape(p.prod)
        desc, shape = cc.operator_desc("f16x3", **_producer_kw(p, p.split_k, True))
        return (p.cout, desc), shape[1:]

    rows = [(f"test_merged_finalise[{fid}]", fid, prods, mode, groups) for fid, prods, mode, groups in trs.FINALISE_ROWS]
    rows += [("test_merged_finalise_of_tile_partials", "tile-partials", (trs.TILE_PRODUCER,), mode, groups) for mode, groups in trs.TILE_MODES]
    for cid, fid, prods, mode, groups in rows:
        if fid in without_rows:
            continue
        parts = [part(p) for p in prods]
        assert len({shape for _, shape in parts}) == 1, f"{fid}: the parts of a concatenation have one spatial extent"
        assert sum(c for (c, _), _ in parts) % groups == 0, fid
        out.setdefault(cc.finalise_class(mode, [pd for pd, _ in parts], groups), []).append(cid)
    return out


def _producer_shape(prod):
    return cc.operator_desc("f16x3", **_producer_kw(prod, prod.split_k, True))[1][1:]


def product_census():
    """({LaunchClass: [where]}, {ReduceClass: [where]}, {FinaliseClass: [where]}) over every claimed configuration, both
    precisions, sub-pixel on and off; where = configuration/precision/form: layer"""
    convs, reduces, finalises = {}, {}, {}
    for name, cfg in PRODUCT.items():
        for prec in ("f16x3", "f32"):
            for sub in ((True, False) if prec == "f16x3" else (False,)):
                walk = cc.product_walk(cfg, prec, sub)
                form = f"{name}/{prec}{'' if sub or prec == 'f32' else '/27-tap'}"
                for layer, cls, shape in walk.records:
                    assert cls is not None, (name, layer)      # every claimed configuration runs on the tiled kernels
                    convs.setdefault(cls, []).append(f"{form}: {layer} {shape}")
                for layer, cls, shape in walk.reduces:
                    reduces.setdefault(cls, []).append(f"{form}: {layer} {shape}")
                for layer, cls in walk.finalises:
                    finalises.setdefault(cls, []).append(f"{form}: after {layer}")
    return convs, reduces, finalises


def product_classes():
    """{LaunchClass: [configuration/precision/form: layer]} of product_census"""
    return product_census()[0]


def _fmt(cls):
    return " ".join(f"{k}={v}" for k, v in cls._asdict().items())


@pytest.fixture(scope="module")
def product():
    return product_census()


@pytest.fixture(scope="module")
def census(product):
    return product[0], operator_launches()


def _listing(kind, product, operator):
    """print every product class with where it comes from and which rows have it; -> the lines of those without a row"""
    print(f"{len(product)} product {kind} classes, {len(operator)} operator-test {kind} classes")
    missing = []
    for cls in sorted(product, key=str):
        where, cases = product[cls], operator.get(cls, [])
        print(f"{_fmt(cls)}\n    product ({len(where)}): {where[0]}" + (f" ... {where[-1]}" if len(where) > 1 else "")
              + f"\n    operator ({len(cases)}): {', '.join(cases[:3]) or 'NONE'}")
        if not cases:
            missing.append(f"{_fmt(cls)}  <- {where[0]}")
    return missing


def test_every_product_launch_class_has_an_operator_test(census):
    product, operator = census
    print(f"{len(product)} product launch classes, {len(operator)} operator-test launch classes")
    missing = []
    for cls in sorted(product, key=str):
        layers, cases = product[cls], operator.get(cls, [])
        print(f"{_fmt(cls)}\n    product ({len(layers)}): {layers[0]}" + (f" ... {layers[-1]}" if len(layers) > 1 else "")
              + f"\n    operator ({len(cases)}): {', '.join(cases[:3]) or 'NONE'}")
        if not cases:
            missing.append(f"{_fmt(cls)}  <- {layers[0]}")
    assert not missing, "product launch classes without an operator test:\n" + "\n".join(missing)


def test_every_instantiation_has_an_operator_test(census):
    """each of the twelve <KS, MB, NB>: unsplit on the exact and the f16x3 path, split on the f16x3 path"""
    _, operator = census
    have = {(c.path, c.ks, c.mb, c.nb, c.split) for c in operator if c.up != "sub-pixel"}
    missing = []
    for ks, mb, nb in INSTANTIATIONS:
        name = f"<{ks},{mb},{nb}>"
        for path, split in (("f32", False), ("f16x3", False), ("f16x3", True)):
            if split and name in UNREACHABLE_SPLIT:
                print(f"{name} split: unreachable -- {UNREACHABLE_SPLIT[name]}")
                continue
            if (path, ks, mb, nb, split) not in have:
                missing.append(f"{name} {path} {'split' if split else 'unsplit'}")
    assert not missing, missing
    assert not any(c.path == "f32" and c.split for c in operator)      # the exact path never splits


def test_census_notices_a_deleted_row():
    """the census depends on single rows of the new table: without g0 (or without k3-64to32-split) a product launch class
    (an instantiation) has no operator test"""
    product = product_classes()
    without = operator_launches(without_rows=("g0",))
    assert [cls for cls in product if cls not in without]
    without = operator_launches(without_rows=("k3-64to32-split",))
    assert ("f16x3", 3, 1, 2, True) not in {(c.path, c.ks, c.mb, c.nb, c.split) for c in without}
    # the reduce and the finalise rows: without res-64to64-4x4x4 the residual reduce of golden_odd13's 4^3 level (one ragged
    # segment, vector form, two slices) has no row; without layernorm-cat-segments-tiles-odd9 the mixed concatenation has none
    _, reduces, finalises = product_census()
    assert not [cls for cls in reduces if cls not in operator_reduces()]
    gap = [cls for cls in reduces if cls not in operator_reduces(without_rows=("res-64to64-4x4x4",))]
    assert gap == [cc.ReduceClass(True, "vector", "1", True, True, "2")], gap
    assert not [cls for cls in finalises if cls not in operator_finalises()]
    gap = [cls for cls in finalises if cls not in operator_finalises(without_rows=("layernorm-cat-segments-tiles-odd9",))]
    assert gap == [cc.FinaliseClass("layernorm", (("segment", "<=256"), ("tile", "<=256", False)), False)], gap


def test_every_product_reduce_class_has_an_operator_test(product):
    """every class of split-K reduce the networks launch has a row in tests/test_splitk_reduce_stats_hip.REDUCE_ROWS"""
    missing = _listing("reduce", product[1], operator_reduces())
    assert not missing, "product reduce classes without an operator test:\n" + "\n".join(missing)


def test_every_product_finalise_class_has_an_operator_test(product):
    """every class of finalise launch the networks issue has a row in tests/test_splitk_reduce_stats_hip.FINALISE_ROWS"""
    missing = _listing("finalise", product[2], operator_finalises())
    assert not missing, "product finalise classes without an operator test:\n" + "\n".join(missing)


def test_both_reduce_forms_have_one_several_and_ragged_segments():
    """splitk_reduce_stats_kernel<true> and <false>: a row with one segment per channel, one with several, and one whose last of
    several segments is ragged -- whether a network reaches it or not; more than 256 segments are unreachable (by name)"""
    have = operator_reduces()
    missing = []
    for form in ("vector", "scalar"):
        mine = [c for c in have if c.stats and c.form == form]
        for what, ok in (("one segment", any(c.segments == "1" for c in mine)), ("several segments", any(c.segments != "1" for c in mine)),
                         ("a ragged last segment of several", any(c.segments != "1" and c.ragged for c in mine))):
            print(f"{form} form, {what}: {'yes' if ok else 'NO'}")
            if not ok:
                missing.append(f"{form} form: {what}")
    assert not missing, missing
    assert not any(c.segments == ">256" for c in have) and "segments>256" in trs.UNREACHABLE_REDUCE
    print(f"segments > 256: unreachable -- {trs.UNREACHABLE_REDUCE['segments>256']}")
    assert not any(k[0] == "segment" and k[1] == ">256" for c in operator_finalises() for k in c.parts) and "segment>256" in trs.UNREACHABLE_FINALISE


def test_no_descriptor_splits_beyond_256_segments():
    """what UNREACHABLE_REDUCE says, asked of the library: with more than 256 * 4096 output voxels no launch splits, however few
    output channels (one column of workgroups) and however many input chunks it has -- for both kernel sizes and the up-conv forms"""
    lay = cc.stats_layout(cc.operator_desc("f16x3", (256,), 256, (16, 16, 16), 3, stats=True, split_stats=True)[0])
    limit = 256 * lay["segment"]
    for dims in ((102, 102, 102), (64, 128, 129), (1, 1024, 1025)):
        assert dims[0] * dims[1] * dims[2] > limit
        for cout in (8, 32, 64):
            for k in (1, 3):
                desc, shape = cc.operator_desc("f16x3", (256,), cout, dims, k, stats=True, split_stats=True)
                assert cc.tile_geometry(desc)["slices"] == 1 and not desc.d_workspace, (dims, cout, k)
    for sub in (True, False):       # the smallest up-conv output beyond the limit comes from a stored tensor an eighth of it
        desc, shape = cc.operator_desc("f16x3", (256,), 8, (51, 51, 51), 3, upsample=True, subpixel=sub, stats=True, split_stats=True)
        assert shape[1] * shape[2] * shape[3] > limit and cc.tile_geometry(desc)["slices"] == 1, (sub, shape)


def test_the_stand_in_takes_the_product_route():
    """RecordingOps cannot send UNetRunner down another branch than HipOps: every attribute pixie_amd/unet.py probes on its
    operators exists on both or on neither, conv takes the same keywords, and a walk sees the reduce statistics and the merged finalise"""
    probes = set(re.findall(r'hasattr\((?:self\.)?ops,\s*"(\w+)"\)', inspect.getsource(unet_module)))
    print(f"attributes pixie_amd/unet.py probes on its operators: {sorted(probes)}")
    assert "stats_norm_finalize" in probes and len(probes) >= 4, probes         # the scan itself still finds them
    differ = [p for p in sorted(probes) if hasattr(cc.RecordingOps, p) != hasattr(HipOps, p)]
    assert not differ, f"probed attributes HipOps and RecordingOps do not share: {differ}"

    def keywords(fn):
        return {n: p.default for n, p in inspect.signature(fn).parameters.items() if n != "self"}

    for name in ("conv", "stats_finalize", "stats_norm_finalize", "norm_finalize"):
        mine, theirs = keywords(getattr(cc.RecordingOps, name)), keywords(getattr(HipOps, name))
        assert mine == theirs, f"RecordingOps.{name} and HipOps.{name} differ in {sorted(set(mine.items()) ^ set(theirs.items()), key=str)}"
    walk = cc.product_walk(PRODUCT["baseline2_128_seg"], "f16x3", True)
    assert any(cls.stats for _, cls, _ in walk.reduces), "no split launch takes its statistics in the reduce"
    assert any(cls.mode != "sums" for _, cls in walk.finalises), "no merged finalise (pixie_stats_norm_finalize) was seen"
    split = [cls for _, cls, _ in walk.records if cls.split]
    assert len(split) == len(walk.reduces) and not any(cls.stats for cls in split)      # one reduce per split launch; it has the statistics


def test_float64_bound_holds_for_the_reference_alone():
    """the float64 bound of tests/test_splitk_reduce_stats_hip.py, 4 n 2^-53 sum|x|, against the test's own reference: torch's float64
    sum of one channel of 64^3 float32 values and math.fsum (exactly rounded) differ by a small part of it"""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(64 ** 3, generator=g) + 1.5).double()
    b1, b2 = trs.sum_bounds(x.reshape(1, -1))
    e1 = abs(float(x.sum()) - math.fsum(x.tolist()))
    e2 = abs(float((x * x).sum()) - math.fsum((x * x).tolist()))
    print(f"reference alone: |err| / bound {e1 / float(b1):.2e} (sum) {e2 / float(b2):.2e} (squares); one voxel of 1.5 is {1.5 / float(b1):.1e} bounds")
    assert e1 <= 0.25 * float(b1) and e2 <= 0.25 * float(b2)
    assert 1.5 > 1e3 * float(b1)        # a dropped or doubled voxel is far outside
