"""Census of convolution launch classes (CPU only, nothing is launched): every class the product's networks issue has an
operator test, and every one of the twelve kernel instantiations has one -- unsplit on both paths, split on the f16x3 path.

The class of a launch (tests/_conv_census.py) is read from the library's own selection code through pixie_conv_kernel_variant and
pixie_conv_tile_geometry on the descriptor pixie_amd.unet.fill_conv_desc builds, for the product (the plan of every claimed
configuration, walked with a recording stand-in for HipOps) and for the operator tests (their case tables).  A change of the
tile heuristic or of a network plan that opens a gap fails here, naming the layer; so does deleting a row of
tests/test_conv_variants_hip.VARIANT_CASES that a product class depends on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_census as cc                      # noqa: E402
import test_conv_subpixel_hip as tsub          # noqa: E402
import test_conv_variants_hip as tvar          # noqa: E402
import test_unet_hip as tu                     # noqa: E402
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
    return out


def product_classes():
    """{LaunchClass: [configuration/precision/form: layer]} over every claimed configuration, both precisions, sub-pixel on and off"""
    out = {}
    for name, cfg in PRODUCT.items():
        for prec in ("f16x3", "f32"):
            for sub in ((True, False) if prec == "f16x3" else (False,)):
                for layer, cls, shape in cc.product_launches(cfg, prec, sub):
                    assert cls is not None, (name, layer)      # every claimed configuration runs on the tiled kernels
                    label = f"{name}/{prec}{'' if sub or prec == 'f32' else '/27-tap'}: {layer} {shape}"
                    out.setdefault(cls, []).append(label)
    return out


def _fmt(cls):
    return " ".join(f"{k}={v}" for k, v in cls._asdict().items())


@pytest.fixture(scope="module")
def census():
    return product_classes(), operator_launches()


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
