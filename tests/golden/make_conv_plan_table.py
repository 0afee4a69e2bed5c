#!/usr/bin/env python
"""Writes tests/golden/conv_plan_table.json: what the conv launcher's size queries and diagnostics answer, descriptor by descriptor.

Recorded results of the library's own host functions (the PIXIE_DIAG build; no device needed), taken at the commit BEFORE the
launcher was rebuilt around one launch plan; tests/test_conv_plan_table.py holds every later commit to them.  Run it again only
to pin a deliberate change of the tile heuristic, and say so in that commit.

A row is the descriptor's shape fields and flags (COLUMNS up to `skip`; a flag stands for "this pointer is given", and a row
without d_w16 has d_w) and the answers:
pixie_conv_kernel_variant and its slices, the 10 values of pixie_conv_tile_geometry (null: refused), pixie_conv_stats_floats
with and without d_out_stats / d_out_amax, pixie_conv_workspace_bytes, the 6 values of pixie_conv_stats_layout (null: refused),
pixie_conv_skip_foldable -- and `accepted`: does pixie_conv3d_forward launch this descriptor, its operand pointers (inputs, output,
bias, |x|max slots or in_bound, the folded skip's operands) taken as present and no spatial affine.  The rules, from its PX_REQUIRE:

* ksize 1 or 3, stride 1 or 2, upsample 0 or 1, positive sizes, one of d_w / d_w16;
* with d_w16 (f16x3 path): stride 1, or stride 2 with ksize 3 and no upsample; c0 + c1 a multiple of 16 and c0 of 8; w16_subpixel
  only with upsample, ksize 3, stride 1 and no folded skip; a folded skip only where pixie_conv_skip_foldable says 1 (stride 1, no
  upsample, skip channels a positive multiple of 16 with skip_c0 a multiple of 8, an unsplit launch); the staged tile, 64 B per
  halo voxel, within 160 KB of LDS;
* without d_w16: no folded skip; where c0 + c1 is a multiple of 16 and the stride rule above holds the exact tiled launch, with the
  same LDS rule; every other shape goes to the first-generation kernel, whose own LDS limit is not evaluated here (every answer
  recorded for such a row says "not this path" whether it is accepted or not).

Rows: (a) every launch tests/_conv_census.product_walk records for the configurations of tests/test_conv_variant_census.py,
(b) every descriptor the operator tables of test_conv_variants_hip / test_splitk_reduce_stats_hip / test_conv_subpixel_hip (and
the older tables the census reads) build, (c) a seeded sample of SWEEP_ROWS rows of the product
c_in {16, 32, 48+16, 64, 128, 24} x c_out {3, 16, 32, 33, 64, 96, 192} x 15 cubes and 3 anisotropic shapes x ksize {1, 3} x
stride {1, 2} x {no upsample, upsample, upsample + sub-pixel weights} x workspace x crop by one voxel x d_w16 or d_w x folded skip
(218 k rows in full: thinned to keep the file near 100 KB; four rows per line)."""
import ctypes as C
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository

from pixie_amd import _lib      # noqa: E402

SHAPE = ("c0", "c1", "c_out", "in_d", "in_h", "in_w", "ksize", "stride", "upsample", "out_d", "out_h", "out_w", "skip_c0", "skip_c1")
FLAGS = ("w16", "subpixel", "workspace", "skip")     # d_w16 given (else d_w), w16_subpixel, d_workspace given, d_skip_w16 given
ANSWERS = ("variant", "slices", "geometry", "stats_floats_asked", "stats_floats", "workspace_bytes", "layout", "foldable", "accepted")
COLUMNS = SHAPE + FLAGS + ANSWERS
SWEEP_ROWS = 500
OUT = os.path.join(HERE, "conv_plan_table.json")


def descriptor(row, stats=False):
    """the pixie_conv_desc of a row (dict or sequence in COLUMNS order): 1 stands for every pointer that is given"""
    r = row if isinstance(row, dict) else dict(zip(COLUMNS, row))
    d = _lib.ConvDesc()
    for k in SHAPE:
        setattr(d, k, int(r[k]))
    d.w16_subpixel = int(r["subpixel"])
    d.d_in0 = d.d_out = d.d_bias = 1
    d.d_in1 = 1 if r["c1"] else None
    d.d_w16 = 1 if r["w16"] else None
    d.d_w = None if r["w16"] else 1
    d.d_in_amax0 = 1 if r["w16"] else None
    d.d_in_amax1 = 1 if r["w16"] and r["c1"] else None
    d.d_workspace = 1 if r["workspace"] else None
    if r["skip"]:
        d.d_skip_w16 = d.d_skip_in0 = d.d_skip_amax0 = d.d_skip_bias = 1
        d.d_skip_in1 = d.d_skip_amax1 = 1 if r["skip_c1"] else None
    if stats:
        d.d_out_stats = d.d_out_amax = 1
    return d


def answers(lib, row):
    """the library's answers for a row, in ANSWERS order without `accepted`"""
    d = descriptor(row)
    sl = C.c_int(1)
    variant = int(lib.pixie_conv_kernel_variant(C.byref(d), C.byref(sl)))
    geo = (C.c_int32 * 10)()
    geo = [int(v) for v in geo] if lib.pixie_conv_tile_geometry(C.byref(d), geo) == 0 else None
    lay = (C.c_int64 * 6)()
    lay = [int(v) for v in lay] if lib.pixie_conv_stats_layout(C.byref(d), lay) == 0 else None
    return [variant, int(sl.value), geo, int(lib.pixie_conv_stats_floats(C.byref(descriptor(row, True)))),
            int(lib.pixie_conv_stats_floats(C.byref(descriptor(row, False)))), int(lib.pixie_conv_workspace_bytes(C.byref(d))), lay,
            int(lib.pixie_conv_skip_foldable(C.byref(d)))]


def accepted(r, ans):
    """pixie_conv3d_forward's rules (module docstring), from the row and the answers recorded for it"""
    geo, foldable = ans[2], ans[7]
    cin = r["c0"] + r["c1"]
    if r["ksize"] not in (1, 3) or r["stride"] not in (1, 2) or r["upsample"] not in (0, 1):
        return False
    if min(r["c0"], r["c_out"], r["in_d"], r["in_h"], r["in_w"]) <= 0 or r["c1"] < 0:
        return False
    strided_ok = r["stride"] == 1 or (r["ksize"] == 3 and not r["upsample"])
    sub = bool(r["w16"] and r["subpixel"])
    if r["w16"]:
        if not strided_ok or cin % 16 or r["c0"] % 8:
            return False
        if sub and not (r["upsample"] == 1 and r["ksize"] == 3 and r["stride"] == 1 and not r["skip"]):
            return False
        if r["skip"] and not foldable:
            return False
    else:
        if r["skip"]:
            return False
        if cin % 16 or not strided_ok:
            return True         # first-generation kernel
    tx, ty, tz = geo[:3]
    halo = (tx + 2) * (ty + 1) * (tz + 1) if sub else \
        ((tx - 1) * r["stride"] + r["ksize"]) * ((ty - 1) * r["stride"] + r["ksize"]) * ((tz - 1) * r["stride"] + r["ksize"])
    return 64 * halo <= 160 * 1024


def census_rows():
    """(a) and (b): every descriptor the census builds for the product walks and the operator tables"""
    import _conv_census as cc
    import test_conv_variant_census as census
    seen = []
    fill = cc.fill_conv_desc

    def recording(*a, **kw):
        res = fill(*a, **kw)
        d = res[0]
        r = {k: int(getattr(d, k)) for k in SHAPE}
        assert bool(d.d_w16) != bool(d.d_w)
        r.update(w16=int(bool(d.d_w16)), subpixel=int(d.w16_subpixel), workspace=int(bool(d.d_workspace)), skip=int(bool(d.d_skip_w16)))
        seen.append(tuple(r[k] for k in SHAPE + FLAGS))
        return res

    cc.fill_conv_desc = recording
    try:
        census.product_census()
        census.operator_launches()
        census.operator_reduces()
        census.operator_finalises()
    finally:
        cc.fill_conv_desc = fill
    return seen


def sweep_rows():
    """(c), thinned: a seeded sample of the full product"""
    cins = ((16, 0), (32, 0), (48, 16), (64, 0), (128, 0), (24, 0))
    couts = (3, 16, 32, 33, 64, 96, 192)
    shapes = [(e, e, e) for e in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 64, 128)] + [(1, 1, 4096), (5, 33, 64), (64, 9, 2)]
    ups = ((0, 0), (1, 0), (1, 1))          # (upsample, sub-pixel weights)
    full = list(itertools.product(cins, couts, shapes, (1, 3), (1, 2), ups, (0, 1), (0, 1), (0, 1), (0, 1)))
    rows = []
    for (c0, c1), cout, (d, h, w), k, stride, (up, sub), ws, crop, w16, skip in random.Random(20261018).sample(full, SWEEP_ROWS):
        pad = 1 if k == 3 else 0
        nat = [((n << up) + 2 * pad - k) // stride + 1 for n in (d, h, w)]
        od, oh, ow = [max(1, n - 1) for n in nat] if crop else (0, 0, 0)
        rows.append((c0, c1, cout, d, h, w, k, stride, up, od, oh, ow, 32 if skip else 0, 0,
                     w16, sub, ws, skip))
    return rows


def main():
    lib = _lib.load(diag=True)
    keys = list(dict.fromkeys(census_rows() + sweep_rows()))
    rows = []
    for key in keys:
        r = dict(zip(SHAPE + FLAGS, key))
        ans = answers(lib, r)
        rows.append(list(key) + ans + [int(accepted(r, ans))])
    with open(OUT, "w") as f:
        f.write('{"columns": ' + json.dumps(COLUMNS) + ',\n "rows": [\n' + ",\n".join(",".join(json.dumps(r, separators=(",", ":")) for r in rows[i:i + 4]) for i in range(0, len(rows), 4)) + "\n]}\n")
    n_acc = sum(r[-1] for r in rows)
    print(f"{OUT}: {len(rows)} rows ({n_acc} accepted, {len(rows) - n_acc} refused), {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
