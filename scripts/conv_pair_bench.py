#!/usr/bin/env python
"""Pair form against 4-wave form of the f16x3 convolution launches with 128 or more output channels that a 128^3 scene issues.

Each class is ONE descriptor, launched through libpixie_hip_diag.so in the form the launcher picks (pair) and with the diag switch
that keeps the 4-wave kernels, alternately: HIP events around `launches` back-to-back launches, `timings` such timings per form
(the first holds the clock ramp), us per launch; "steady" is the mean of timings 2 .. n.  Random operands, in_bound 64, the
split-K classes with their workspace (their figure includes the reduce, which is the same kernel in both forms).
Usage: conv_pair_bench.py [timings] [launches]"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixie_amd import _lib                                     # noqa: E402
from pixie_amd.unet import ACT_SILU, HipOps, fill_conv_desc    # noqa: E402

CLASSES = [  # (name, c_in, c_out, D, ksize, norm + SiLU prologue)
    ("projector 128->128 3^3 at 128^3, SiLU prologue", 128, 128, 128, 3, True),
    ("128->128 3^3 at 32^3 (split-K 4)", 128, 128, 32, 3, False),
    ("256->256 3^3 at 16^3 (split-K 8)", 256, 256, 16, 3, False),
    ("64->128 1x1x1 at 128^3", 64, 128, 128, 1, False),
    ("128->128 1x1x1 at 32^3 (split-K 4)", 128, 128, 32, 1, False),
    ("256->256 1x1x1 at 16^3 (split-K 8)", 256, 256, 16, 1, False),
]


def main():
    timings = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    ops = HipOps(dev)
    lib = _lib.load(diag=True)
    g = torch.Generator().manual_seed(0)

    def switch(on):
        v = C.c_int(1 if on else 0)
        lib.pixie_conv_kernel_variant(None, C.byref(v))

    for name, cin, cout, D, k, prologue in CLASSES:
        x = torch.randn((cin, D, D, D), generator=g).to(dev)
        w = (torch.randn((cout, cin, k, k, k), generator=g) / (cin * k ** 3) ** 0.5).to(dev)
        b = torch.randn(cout, generator=g).to(dev)
        kw = dict(w16=ops.pack_conv16(w), split_k=True)
        if prologue:
            kw.update(pro=(torch.ones(cin, device=dev), torch.zeros(cin, device=dev)), act=ACT_SILU, in_bound=64.0)
        else:
            slot = torch.zeros(1, dtype=torch.int32, device=dev)
            ops.channel_stats(x, slot)
            kw["in_amax"] = [slot]
        desc, out, _, ws = fill_conv_desc(lib, lambda s, d: torch.empty(s, device=dev, dtype=d), [x], None, b, cout, k, **kw)
        sl = C.c_int(1)
        variant = lib.pixie_conv_kernel_variant(C.byref(desc), C.byref(sl))
        switch(False)
        lds = lib.pixie_conv_tile_geometry(C.byref(desc), None)
        print(f"{name}: variant {variant} x{sl.value}, pair-form LDS {lds} B", flush=True)
        res = {"pair": [], "4-wave": []}
        outs = {}
        for _ in range(timings):
            for form in ("4-wave", "pair"):
                switch(form == "4-wave")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    _lib.check(lib.pixie_conv3d_forward(C.byref(desc), _lib.current_stream_ptr()), "pixie_conv3d_forward")
                e1.record()
                torch.cuda.synchronize()
                res[form].append(e0.elapsed_time(e1) * 1000.0 / launches)
                outs[form] = out.clone()
        switch(False)
        steady = {f: sum(v[1:]) / max(1, len(v) - 1) for f, v in res.items()}
        for f in ("4-wave", "pair"):
            print(f"    {f:7s} " + " ".join(f"{t:8.1f}" for t in res[f]) + f"    steady {steady[f]:8.1f}", flush=True)
        print(f"    pair - 4-wave = {steady['pair'] - steady['4-wave']:+.1f} us = {100.0 * (steady['pair'] / steady['4-wave'] - 1.0):+.2f} %;"
              f" outputs byte-equal: {torch.equal(outs['pair'].view(torch.int32), outs['4-wave'].view(torch.int32))}", flush=True)
        del x, w, out, ws, outs


if __name__ == "__main__":
    main()
