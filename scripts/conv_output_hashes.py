#!/usr/bin/env python
"""SHA-256 of what HipOps.conv writes for every row of tests/test_conv_variants_hip.VARIANT_CASES: one line per launch.

For comparing two builds of the library bit for bit (a refactoring of the launcher must leave every line as it was): the inputs
come from a seeded CPU generator, every launch the row's test makes is made once (tests/test_conv_variants_hip.launches: split or
not, statistics or not; a split row also once with the statistics taken in its reduce), and the line carries the hash of the output
bytes and, where statistics were asked for, of the finalised float64 sums and of the |x|max slot.  The conv path has no
floating-point atomics and the split-K reduce adds in a fixed order, so two runs of one build print the same listing.
Usage: conv_output_hashes.py [row id ...]"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_conv_variants_hip as tvar      # noqa: E402
from pixie_amd.unet import HipOps          # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def inputs(case, seed):
    g = torch.Generator().manual_seed(seed)
    dims = tuple(case.dims)
    cin = sum(case.cins)
    parts = [torch.randn((c,) + dims, generator=g) * (1.0 + 3.0 * i) + (3.0 if i == 0 else 0.0) for i, c in enumerate(case.cins)]
    w = torch.randn((case.cout, cin) + (case.k,) * 3, generator=g) / np.sqrt(cin * case.k ** 3)
    b = torch.randn(case.cout, generator=g)
    pro = (torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)) if case.pro != "none" else None
    affine = (torch.randn(dims, generator=g), torch.randn(dims, generator=g)) if case.pro == "channel+spatial" else None
    skip = None
    if case.skip:
        skip = ([torch.randn((c,) + dims, generator=g) for c in case.skip],
                torch.randn((case.cout, sum(case.skip), 1, 1, 1), generator=g) / np.sqrt(sum(case.skip)), torch.randn(case.cout, generator=g))
    return parts, w, b, pro, affine, skip, g


def main():
    dev = torch.device("cuda:0")
    ops = HipOps(dev)
    to = lambda t: t.to(dev) if t is not None else None
    want = set(sys.argv[1:])
    for idx, case in enumerate(tvar.VARIANT_CASES):
        if want and case.id not in want:
            continue
        parts, w, b, pro, affine, skip, g = inputs(case, 5000 + idx)
        dparts = [to(p) for p in parts]
        up = case.up != "none"
        kw = dict(stride=case.stride, upsample=up, pro=tuple(map(to, pro)) if pro else None, affine=tuple(map(to, affine)) if affine else None,
                  act=case.act)
        if case.out_size is not None:
            kw["out_size"] = tuple(case.out_size)
        residual = None
        for prec in tvar.runs(case):
            todo = list(tvar.launches(case, prec))
            if prec == "f16x3" and len(todo) == 2 and todo[0] == (True, False) and todo[1] == (False, True):
                todo.append((True, True))      # a split row: the reduce takes the statistics
            k = dict(kw)
            if prec == "f32":
                packed = ops.pack_conv(to(w))
            else:
                packed = None
                sub = case.up == "sub-pixel"
                k["w16"] = ops.pack_conv_subpixel(to(w)) if sub else ops.pack_conv16(to(w))
                k["subpixel"] = sub
                if pro is not None:
                    k["in_bound"] = 2.0 * float(tvar._prologue_cpu(parts, pro, affine, case.act).abs().max())
                else:
                    k["in_amax"] = tvar._amax_slots(ops, dparts)
                if skip is not None:
                    dxs = [to(x) for x in skip[0]]
                    k["skip"] = dict(parts=dxs, w16=ops.pack_conv16(to(skip[1])), bias=to(skip[2]), amax=tvar._amax_slots(ops, dxs))
            for sk, stats in todo:
                ops.split_k = sk
                slot = torch.zeros(1, dtype=torch.int32, device=dev) if stats else None
                if case.res and residual is None:
                    shape = tvar.operator_desc(prec, case.cins, case.cout, case.dims, case.k, stride=case.stride, upsample=up,
                                               out_size=case.out_size)[1]
                    residual = to(torch.randn(shape, generator=g))
                res = ops.conv(dparts, packed, to(b), case.cout, case.k, residual=residual, out_amax=slot, defer_stats=stats and sk, **k)
                out, sums = res if stats else (res, None)
                if sums is not None and not torch.is_tensor(sums):
                    sums = ops.stats_finalize(sums)
                torch.cuda.synchronize()
                line = f"{case.id} {prec} split_k={int(sk)} stats={int(stats)} out {sha(out)}"
                if stats:
                    line += f" sums {sha(sums) if sums is not None else '-'} amax {int(slot.item())}"
                print(line, flush=True)


if __name__ == "__main__":
    main()
