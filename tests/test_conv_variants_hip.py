"""GPU operator tests of the convolution launches by KERNEL VARIANT and TILE GEOMETRY rather than by shape.

pixie_conv3d_forward picks, from the shape alone, one of twelve conv3d_f16x3_kernel<KS, MB, NB> instantiations (or the exact-fp32
twins, or the sub-pixel kernel), a split-K factor and a tile.  VARIANT_CASES holds one row per launch class that the product's
networks issue and the older operator tables do not reach (tests/test_conv_variant_census.py computes both sets from the library
and fails when a product launch class has no row here or there), plus the geometries no network has but the tile code must get
right: ragged last tiles behind full ones along x, odd input extents under stride 2, a tile depth that is not a power of two.

Reference: float64 F.conv3d on the CPU over the WHOLE output (test_unet_hip.ref_conv); every row costs under 30 GFLOP (column
`gflop`), so no row needs a slab comparison.  Bounds, the project's own: rel-L2 < 2e-6 (f16x3) / < 1e-5 (exact fp32) against
float64, split-K against the unsplit launch < 1e-6, two launches bit-equal, epilogue statistics against a separate pass < 1e-6 and
|x|max bit-equal.  New here:

* per tile: the same rel-L2 on every tile-shaped block of the output (extents from pixie_conv_tile_geometry) holds the same bound,
  so that an error confined to one ragged or corner tile (1/512 of a 64^3 output) cannot hide in the whole-tensor figure.
  The CPU emulation of the f16x3 arithmetic (tests/_torch_ref_ops.TorchRefOpsF16x3: the arithmetic model, not the code under test)
  against float64 on the 53 f16x3 rows of this table under 1 GFLOP (27-tap form) has a worst tile of 3.63e-7 (row g38; worst
  whole-tensor figure 3.25e-7), under 1e-6, so the per-tile bound is the whole-tensor one, 2e-6.
* epilogue statistics against float64: per-channel sum and sum of squares of the float64 reference output, rtol 1e-5 (atol 1e-3
  on the sum, which may cancel), the bound test_conv3d_folded_skip_convolution uses.

The bias of every channel has the sign of that channel's mean output.  The relative error of a sum is a statement about the
summation only where the sum is well conditioned; where a channel's mean cancels, it is the convolution's own rounding -- inside
its per-element bound, but systematic along a channel, because the split error of a weight is the same at every voxel --
multiplied by the condition number sum|y| / |sum y|.  Measured with a bias of random sign (21 of 204 runs missed the bound on the
sum, worst channel 4.7e-4 at c_out = 2048, while the sum of squares, which cannot cancel, stayed below 1.6e-6 everywhere): that
figure said nothing about the epilogue, so the data keep the sums away from cancellation instead.

Inputs are Gaussian with a per-part magnitude spread (1, 4, ...) and a constant offset of 3 sigma on the first part: a tile whose
halo is read from the wrong plane cannot hide in zero-mean noise."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from _conv_census import operator_desc, tile_geometry
from test_unet_hip import _amax_slots, _prologue_cpu, ref_conv, rel_l2

pytestmark = pytest.mark.gpu

TOL = {"f16x3": 2e-6, "f32": 1e-5}
PER_TILE_TOL = {"f16x3": 2e-6, "f32": 1e-5}

# prec: which paths run the row ("both", or the one path whose launch class the row is there for)
# up: "none" | "27-tap" | "sub-pixel" (sub-pixel rows run on the f16x3 path only: the exact path has no such kernel)
# pro: "none" | "channel" (norm scale/shift per channel) | "channel+spatial" (+ LayerNorm gamma/beta per voxel); act 0 none, 1 LeakyReLU, 2 SiLU
# skip: channel counts of the folded 1x1x1 skip convolution's inputs (f16x3 only) or None; split_k: HipOps.split_k for the launch
VC = namedtuple("VC", "id prec cins cout dims k stride up pro act res out_size skip split_k gflop")

VARIANT_CASES = [
    VC("pw128to64", "both", (128,), 64, (64, 64, 64), 1, 1, "none", "none", 0, False, None, None, True, 4.29),   # 1x1x1 at 64^3: <1,2,4>
    VC("pw64+64to64", "both", (64, 64), 64, (64, 64, 64), 1, 1, "none", "none", 0, False, None, None, True, 4.29),   # 1x1x1 on a concatenated input at 64^3
    VC("projtail", "both", (128,), 32, (64, 64, 64), 1, 1, "none", "channel", 2, False, None, None, True, 2.15),   # projector tail: GroupNorm + SiLU prologue, <1,1,4>
    VC("pw32to64", "both", (32,), 64, (32, 64, 64), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,2>
    VC("pw64to32", "both", (64,), 32, (32, 32, 64), 1, 1, "none", "none", 0, False, None, None, True, 0.27),   # <1,1,2>, split in two
    VC("pw64to128-nosplit", "both", (64,), 128, (16, 16, 16), 1, 1, "none", "none", 0, False, None, None, False, 0.07),   # too few workgroups, no workspace: MB falls back to 1, <1,1,1> unsplit
    VC("qkv4096", "both", (256,), 768, (1, 1, 4096), 1, 1, "none", "channel", 0, False, None, None, True, 1.61),   # attention qkv: one row of 128 x tiles; <1,2,4> split in eight
    VC("qkv4096-nosplit", "f16x3", (256,), 768, (1, 1, 4096), 1, 1, "none", "channel", 0, False, None, None, False, 1.61),   # ... <1,1,1> with splitting off
    VC("qkv1000", "both", (256,), 768, (1, 1, 1000), 1, 1, "none", "channel", 0, False, None, None, True, 0.39),   # T = 1000: ragged end of the row; <1,2,1> split in eight
    VC("qkv1000-nosplit", "f16x3", (256,), 768, (1, 1, 1000), 1, 1, "none", "channel", 0, False, None, None, False, 0.39),
    VC("head8", "both", (64,), 8, (64, 64, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 7.25),   # head 64 -> 8 at 64^3: <3,1,4>
    VC("head3", "both", (64,), 3, (64, 64, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 2.72),   # head 64 -> 3
    VC("k3-32to8", "both", (32,), 8, (32, 64, 64), 3, 1, "none", "none", 0, False, None, None, True, 1.81),   # <3,1,2>
    VC("k3-32to64", "both", (32,), 64, (32, 64, 64), 3, 1, "none", "none", 0, False, None, None, True, 14.5),   # <3,2,2> unsplit
    VC("down64", "both", (64,), 128, (64, 64, 64), 3, 2, "none", "none", 0, False, None, None, True, 14.5),   # stride 2, unsplit, 256 full tiles
    VC("down33x34x35", "both", (64,), 64, (33, 34, 35), 3, 2, "none", "none", 0, False, None, None, True, 1.15),   # stride 2 from odd and even extents, split in two
    VC("down13", "both", (64,), 64, (13, 13, 13), 3, 2, "none", "none", 0, False, None, None, True, 0.08),   # 13 -> 7: TZ = 7, not a power of two
    VC("down9", "both", (64,), 64, (9, 9, 9), 3, 2, "none", "none", 0, False, None, None, True, 0.03),   # 9 -> 5
    VC("down32-split", "both", (128,), 128, (32, 32, 32), 3, 2, "none", "none", 0, False, None, None, True, 3.62),   # stride 2, split-K
    VC("k3-256to32-split", "both", (256,), 32, (32, 32, 32), 3, 1, "none", "none", 0, False, None, None, True, 14.5),   # <3,1,4> split in eight (f16x3)
    VC("pw256to32-split", "both", (256,), 32, (32, 32, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,1,4> split in eight (f16x3)
    VC("k3-64to32-split", "both", (64,), 32, (16, 64, 64), 3, 1, "none", "none", 0, False, None, None, True, 7.25),   # <3,1,2> split in two (f16x3)
    VC("pw64to32-nosplit", "both", (64,), 32, (32, 64, 64), 1, 1, "none", "none", 0, False, None, None, False, 0.54),   # <1,1,2> unsplit on both paths
    VC("ragged12x20x40", "both", (64,), 64, (12, 20, 40), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 2.12),   # ragged last x tile behind a full one
    VC("ragged12x20x40-nosplit", "f16x3", (64,), 64, (12, 20, 40), 3, 1, "none", "channel+spatial", 1, True, None, None, False, 2.12),
    VC("ragged9x33x65", "both", (64,), 64, (9, 33, 65), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 4.27),   # ragged last x tile behind a full one
    VC("ragged9x33x65-nosplit", "f16x3", (64,), 64, (9, 33, 65), 3, 1, "none", "channel+spatial", 1, True, None, None, False, 4.27),
    VC("ragged5x6x97", "both", (64,), 64, (5, 6, 97), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.64),   # ragged last x tile behind a full one
    VC("ragged5x6x97-nosplit", "f16x3", (64,), 64, (5, 6, 97), 3, 1, "none", "channel+spatial", 1, True, None, None, False, 0.64),
    VC("ragged40x48x72", "both", (32,), 64, (40, 48, 72), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 15.29),   # ragged x, large enough to stay on an unsplit <3,2,2> tile
    VC("sub11x19x39", "f16x3", (64,), 64, (6, 10, 20), 3, 1, "sub-pixel", "none", 0, False, (11, 19, 39), None, True, 1.8),   # sub-pixel, odd crop, ragged x
    VC("sub11x19x39-nosplit", "f16x3", (64,), 64, (6, 10, 20), 3, 1, "sub-pixel", "none", 0, False, (11, 19, 39), None, False, 1.8),
    VC("sub9x33x65", "f16x3", (64,), 64, (5, 17, 33), 3, 1, "sub-pixel", "none", 0, False, (9, 33, 65), None, True, 4.27),   # sub-pixel, odd crop, ragged x
    VC("sub9x33x65-nosplit", "f16x3", (64,), 64, (5, 17, 33), 3, 1, "sub-pixel", "none", 0, False, (9, 33, 65), None, False, 4.27),
    VC("sub5x6x97", "f16x3", (64,), 64, (3, 3, 49), 3, 1, "sub-pixel", "none", 0, False, (5, 6, 97), None, True, 0.64),   # sub-pixel, odd crop, ragged x
    VC("sub5x6x97-nosplit", "f16x3", (64,), 64, (3, 3, 49), 3, 1, "sub-pixel", "none", 0, False, (5, 6, 97), None, False, 0.64),
    VC("fold12x20x40", "f16x3", (64,), 64, (12, 20, 40), 3, 1, "none", "channel+spatial", 1, False, None, (64, 64), False, 2.28),   # folded skip over ragged tiles
    VC("fold9x33x65", "f16x3", (64,), 64, (9, 33, 65), 3, 1, "none", "channel+spatial", 1, False, None, (64, 64), False, 4.59),   # folded skip over ragged tiles
    VC("fold5x6x97", "f16x3", (64,), 64, (5, 6, 97), 3, 1, "none", "channel+spatial", 1, False, None, (64, 64), False, 0.69),   # folded skip over ragged tiles
    VC("g0", "f16x3", (16,), 8, (1, 3, 5), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g1", "f16x3", (64,), 8, (9, 9, 9), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,1,1> split, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g2", "f16x3", (16,), 8, (64, 64, 64), 1, 1, "none", "channel", 2, False, None, None, True, 0.07),   # <1,1,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g3", "f16x3", (16,), 8, (32, 64, 128), 1, 1, "none", "channel", 2, False, None, None, True, 0.07),   # <1,1,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g4", "f16x3", (64,), 64, (1, 1, 2), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,2,1> split, tiles x (1, full) y (1, full) z (1, full)
    VC("g5", "f16x3", (64,), 64, (1, 1, 2), 1, 1, "none", "none", 0, True, None, None, True, 0.0),   # <1,2,1> split, tiles x (1, full) y (1, full) z (1, full)
    VC("g6", "f16x3", (64,), 64, (2, 8, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,2,1> split, tiles x (1, full) y (2, full) z (2, full)
    VC("g7", "f16x3", (64,), 64, (2, 8, 32), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,2,1> split, tiles x (1, full) y (2, full) z (2, full)
    VC("g8", "f16x3", (64,), 64, (1, 3, 5), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g9", "f16x3", (64,), 64, (1, 3, 5), 1, 1, "none", "none", 0, True, None, None, True, 0.0),   # <1,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g10", "f16x3", (64,), 64, (9, 9, 9), 1, 1, "none", "none", 0, False, None, None, True, 0.01),   # <1,2,1> split, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g11", "f16x3", (32, 32), 64, (2, 8, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,2,1> split, tiles x (1, full) y (2, full) z (2, full)
    VC("g12", "f16x3", (32, 32), 64, (3, 12, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.01),   # <1,2,1> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g13", "f16x3", (32, 32), 64, (1, 3, 5), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g14", "f16x3", (64,), 1024, (8, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g15", "f16x3", (64,), 1024, (8, 16, 32), 1, 1, "none", "none", 0, True, None, None, True, 0.54),   # <1,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g16", "f16x3", (32, 32), 1024, (8, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g17", "f16x3", (16,), 2048, (16, 16, 32), 1, 1, "none", "channel", 2, False, None, None, True, 0.54),   # <1,2,4>, tiles x (1, full) y (3, full) z (3, full)
    VC("g18", "f16x3", (16,), 1024, (16, 16, 64), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g19", "f16x3", (16,), 512, (16, 16, 128), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g20", "f16x3", (64,), 2048, (8, 16, 32), 1, 1, "none", "channel", 2, False, None, None, True, 1.07),   # <1,2,4> split, tiles x (1, full) y (3, full) z (2, full)
    VC("g21", "f16x3", (64,), 1024, (16, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 1.07),   # <1,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g22", "f16x3", (64,), 1024, (16, 16, 32), 1, 1, "none", "none", 0, True, None, None, True, 1.07),   # <1,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g23", "f16x3", (32, 32), 1024, (16, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 1.07),   # <1,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g24", "f16x3", (16,), 8, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g25", "f16x3", (16,), 8, (9, 9, 9), 3, 1, "none", "none", 0, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g26", "f16x3", (16,), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g27", "f16x3", (16,), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g28", "f16x3", (16,), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, False, None, (16, 16), True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g29", "f16x3", (16,), 8, (9, 9, 9), 3, 1, "none", "channel", 2, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g30", "f16x3", (16,), 8, (1, 5, 5), 3, 2, "none", "none", 0, False, None, None, True, 0.0),   # <3,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g31", "f16x3", (32, 32), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.02),   # <3,1,1> split, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g32", "f16x3", (16,), 8, (64, 64, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 1.81),   # <3,1,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g33", "f16x3", (16,), 8, (32, 64, 128), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 1.81),   # <3,1,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g34", "f16x3", (16,), 2048, (7, 32, 64), 3, 2, "none", "none", 0, False, None, None, True, 3.62),   # <3,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g35", "f16x3", (16,), 1024, (7, 32, 128), 3, 2, "none", "none", 0, False, None, None, True, 3.62),   # <3,2,1>, tiles x (2, full) y (3, full) z (3, full)
    VC("g36", "f16x3", (16,), 1024, (8, 24, 192), 3, 2, "none", "none", 0, False, None, None, True, 4.08),   # <3,2,1>, tiles x (3, full) y (3, full) z (3, full)
    VC("g37", "f16x3", (64,), 64, (1, 2, 2), 3, 1, "27-tap", "none", 0, False, (1, 3, 3), None, True, 0.0),   # <3,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g38", "f16x3", (64,), 64, (5, 5, 5), 3, 1, "27-tap", "none", 0, False, (9, 9, 9), None, True, 0.16),   # <3,2,1> split, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g39", "f16x3", (64,), 64, (1, 1, 2), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,2,1> split, tiles x (1, full) y (1, full) z (1, full)
    VC("g40", "f16x3", (64,), 64, (2, 8, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.11),   # <3,2,1> split, tiles x (1, full) y (2, full) z (2, full)
    VC("g41", "f16x3", (64,), 64, (2, 8, 32), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.11),   # <3,2,1> split, tiles x (1, full) y (2, full) z (2, full)
    VC("g42", "f16x3", (64,), 64, (3, 12, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.25),   # <3,2,1> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g43", "f16x3", (64,), 64, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.0),   # <3,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g44", "f16x3", (64,), 64, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g45", "f16x3", (64,), 64, (9, 9, 9), 3, 1, "none", "channel", 2, False, None, None, True, 0.16),   # <3,2,1> split, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g46", "f16x3", (32, 32), 64, (2, 8, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.11),   # <3,2,1> split, tiles x (1, full) y (2, full) z (2, full)
    VC("g47", "f16x3", (32, 32), 64, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,2,1> split, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g48", "f16x3", (64,), 64, (1, 1, 2), 3, 2, "none", "none", 0, False, None, None, True, 0.0),   # <3,2,1> split, tiles x (1, full) y (1, full) z (1, full)
    VC("g49", "f16x3", (64,), 64, (5, 24, 64), 3, 2, "none", "none", 0, False, None, None, True, 0.25),   # <3,2,1> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g50", "f16x3", (64,), 1024, (4, 8, 16), 3, 1, "27-tap", "none", 0, False, None, None, True, 14.5),   # <3,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g51", "f16x3", (64,), 1024, (8, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g52", "f16x3", (64,), 1024, (8, 16, 32), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 14.5),   # <3,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g53", "f16x3", (32, 32), 1024, (8, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,2> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g54", "f16x3", (16,), 1024, (8, 8, 32), 3, 1, "27-tap", "none", 0, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g55", "f16x3", (16,), 512, (8, 8, 64), 3, 1, "27-tap", "none", 0, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g56", "f16x3", (16,), 1024, (16, 16, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g57", "f16x3", (16,), 1024, (16, 16, 64), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g58", "f16x3", (16,), 1024, (16, 16, 64), 3, 1, "none", "channel", 2, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g59", "f16x3", (16,), 512, (16, 16, 128), 3, 1, "none", "channel", 2, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g60", "f16x3", (16,), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g61", "f16x3", (16,), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g62", "f16x3", (16,), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, False, None, (16, 16), True, 15.57),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g63", "f16x3", (8, 8), 1024, (16, 16, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g64", "f16x3", (8, 8), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g65", "f16x3", (16,), 64, (8, 12, 64), 3, 1, "sub-pixel", "none", 0, False, None, None, True, 2.72),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g66", "f16x3", (16,), 64, (8, 12, 96), 3, 1, "sub-pixel", "none", 0, False, None, None, True, 4.08),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g67", "f16x3", (128,), 512, (8, 8, 16), 3, 1, "27-tap", "none", 0, False, None, None, True, 28.99),   # <3,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g68", "f16x3", (128,), 512, (16, 16, 32), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 28.99),   # <3,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g69", "f16x3", (128,), 512, (16, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 28.99),   # <3,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g70", "f16x3", (64, 64), 512, (16, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 28.99),   # <3,2,4> split, tiles x (1, full) y (3, full) z (3, full)
    VC("g71", "f16x3", (64,), 64, (1, 8, 2), 3, 1, "sub-pixel", "none", 0, False, None, None, True, 0.03),   # <3,2,4> split, tiles x (1, full) y (2, full) z (1, full)
    VC("g72", "f16x3", (64,), 64, (1, 1, 2), 3, 1, "sub-pixel", "none", 0, False, (1, 1, 3), None, True, 0.0),   # <3,2,4> split, tiles x (1, full) y (1, full) z (1, full)
    VC("g73", "f32", (16,), 8, (1, 1, 2), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (1, full) z (1, full)
    VC("g74", "f32", (16,), 8, (1, 1, 2), 1, 1, "none", "none", 0, True, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (1, full) z (1, full)
    VC("g75", "f32", (16,), 8, (2, 8, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (2, full) z (2, full)
    VC("g76", "f32", (16,), 8, (2, 8, 32), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (2, full) z (2, full)
    VC("g77", "f32", (16,), 8, (2, 8, 32), 1, 1, "none", "none", 0, True, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (2, full) z (2, full)
    VC("g78", "f32", (16,), 8, (3, 12, 32), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g79", "f32", (16,), 8, (3, 12, 32), 1, 1, "none", "none", 0, True, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g80", "f32", (16,), 8, (1, 3, 5), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g81", "f32", (16,), 8, (1, 3, 5), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g82", "f32", (16,), 8, (1, 3, 5), 1, 1, "none", "none", 0, True, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g83", "f32", (16,), 8, (9, 9, 9), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g84", "f32", (16,), 8, (9, 9, 9), 1, 1, "none", "channel", 2, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g85", "f32", (8, 8), 8, (2, 8, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (2, full) z (2, full)
    VC("g86", "f32", (8, 8), 8, (3, 12, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g87", "f32", (8, 8), 8, (1, 3, 5), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g88", "f32", (8, 8), 8, (9, 9, 9), 1, 1, "none", "none", 0, False, None, None, True, 0.0),   # <1,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g89", "f32", (16,), 8, (64, 64, 64), 1, 1, "none", "channel", 2, False, None, None, True, 0.07),   # <1,1,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g90", "f32", (16,), 8, (32, 64, 128), 1, 1, "none", "channel", 2, False, None, None, True, 0.07),   # <1,1,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g91", "f32", (16,), 2048, (4, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.13),   # <1,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g92", "f32", (8, 8), 2048, (4, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.13),   # <1,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g93", "f32", (16,), 2048, (8, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.27),   # <1,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g94", "f32", (16,), 2048, (8, 16, 32), 1, 1, "none", "none", 0, True, None, None, True, 0.27),   # <1,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g95", "f32", (8, 8), 2048, (8, 16, 32), 1, 1, "none", "none", 0, False, None, None, True, 0.27),   # <1,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g96", "f32", (16,), 2048, (16, 16, 32), 1, 1, "none", "channel", 2, False, None, None, True, 0.54),   # <1,2,4>, tiles x (1, full) y (3, full) z (3, full)
    VC("g97", "f32", (16,), 1024, (16, 16, 64), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g98", "f32", (16,), 512, (16, 16, 128), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g99", "f32", (8, 8), 1024, (16, 16, 64), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g100", "f32", (8, 8), 512, (16, 16, 128), 1, 1, "none", "none", 0, False, None, None, True, 0.54),   # <1,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g101", "f32", (16,), 8, (3, 8, 8), 3, 1, "27-tap", "none", 0, False, None, None, True, 0.01),   # <3,1,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g102", "f32", (16,), 8, (1, 2, 2), 3, 1, "27-tap", "none", 0, False, (1, 3, 3), None, True, 0.0),   # <3,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g103", "f32", (16,), 8, (5, 5, 5), 3, 1, "27-tap", "none", 0, False, (9, 9, 9), None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g104", "f32", (16,), 8, (1, 1, 2), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,1,1>, tiles x (1, full) y (1, full) z (1, full)
    VC("g105", "f32", (16,), 8, (2, 8, 32), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.0),   # <3,1,1>, tiles x (1, full) y (2, full) z (2, full)
    VC("g106", "f32", (16,), 8, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g107", "f32", (16,), 8, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.0),   # <3,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g108", "f32", (16,), 8, (9, 9, 9), 3, 1, "none", "none", 0, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g109", "f32", (16,), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g110", "f32", (16,), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g111", "f32", (16,), 8, (9, 9, 9), 3, 1, "none", "channel", 2, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g112", "f32", (8, 8), 8, (2, 8, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,1,1>, tiles x (1, full) y (2, full) z (2, full)
    VC("g113", "f32", (8, 8), 8, (1, 3, 5), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.0),   # <3,1,1>, tiles x (2, ragged) y (2, ragged) z (1, full)
    VC("g114", "f32", (8, 8), 8, (9, 9, 9), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 0.01),   # <3,1,1>, tiles x (2, ragged) y (3, ragged) z (3, ragged)
    VC("g115", "f32", (16,), 8, (1, 1, 2), 3, 2, "none", "none", 0, False, None, None, True, 0.0),   # <3,1,1>, tiles x (1, full) y (1, full) z (1, full)
    VC("g116", "f32", (16,), 8, (5, 24, 64), 3, 2, "none", "none", 0, False, None, None, True, 0.01),   # <3,1,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g117", "f32", (16,), 8, (64, 64, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 1.81),   # <3,1,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g118", "f32", (16,), 8, (32, 64, 128), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 1.81),   # <3,1,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g119", "f32", (16,), 2048, (2, 8, 16), 3, 1, "27-tap", "none", 0, False, None, None, True, 3.62),   # <3,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g120", "f32", (16,), 2048, (4, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 3.62),   # <3,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g121", "f32", (16,), 2048, (4, 16, 32), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 3.62),   # <3,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g122", "f32", (8, 8), 2048, (4, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 3.62),   # <3,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g123", "f32", (16,), 2048, (7, 32, 64), 3, 2, "none", "none", 0, False, None, None, True, 3.62),   # <3,2,1>, tiles x (1, full) y (3, full) z (3, full)
    VC("g124", "f32", (16,), 1024, (7, 32, 128), 3, 2, "none", "none", 0, False, None, None, True, 3.62),   # <3,2,1>, tiles x (2, full) y (3, full) z (3, full)
    VC("g125", "f32", (16,), 1024, (8, 24, 192), 3, 2, "none", "none", 0, False, None, None, True, 4.08),   # <3,2,1>, tiles x (3, full) y (3, full) z (3, full)
    VC("g126", "f32", (16,), 2048, (4, 8, 16), 3, 1, "27-tap", "none", 0, False, None, None, True, 7.25),   # <3,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g127", "f32", (16,), 2048, (8, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 7.25),   # <3,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g128", "f32", (16,), 2048, (8, 16, 32), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 7.25),   # <3,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g129", "f32", (8, 8), 2048, (8, 16, 32), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 7.25),   # <3,2,2>, tiles x (1, full) y (3, full) z (3, full)
    VC("g130", "f32", (16,), 1024, (8, 8, 32), 3, 1, "27-tap", "none", 0, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g131", "f32", (16,), 512, (8, 8, 64), 3, 1, "27-tap", "none", 0, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g132", "f32", (16,), 1024, (16, 16, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g133", "f32", (16,), 1024, (16, 16, 64), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g134", "f32", (16,), 1024, (16, 16, 64), 3, 1, "none", "channel", 2, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g135", "f32", (16,), 512, (16, 16, 128), 3, 1, "none", "channel", 2, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g136", "f32", (16,), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g137", "f32", (16,), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, True, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
    VC("g138", "f32", (8, 8), 1024, (16, 16, 64), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (2, full) y (3, full) z (3, full)
    VC("g139", "f32", (8, 8), 512, (16, 16, 128), 3, 1, "none", "channel+spatial", 1, False, None, None, True, 14.5),   # <3,2,4>, tiles x (3, full) y (3, full) z (3, full)
]


def case_by_id(cid):
    return next(c for c in VARIANT_CASES if c.id == cid)


def runs(case):
    """the paths a row runs on"""
    if case.up == "sub-pixel" or case.skip:
        return ["f16x3"]
    return ["f16x3", "f32"] if case.prec == "both" else [case.prec]


def launches(case, precision):
    """[(split_k, stats)] of the HipOps.conv calls test_conv_variant makes for a row: what the census counts"""
    if precision == "f32":
        return [(True, False)]
    desc, _ = operator_desc("f16x3", case.cins, case.cout, case.dims, case.k, stride=case.stride, upsample=case.up != "none",
                            prologue=case.pro, residual=case.res, out_size=case.out_size, skip_cins=case.skip,
                            subpixel=case.up == "sub-pixel", split_k=case.split_k)
    if tile_geometry(desc)["slices"] > 1:
        return [(True, False), (False, True)]     # split, and the unsplit launch (with statistics) it is compared with
    return [(case.split_k, False), (case.split_k, True)]


@pytest.fixture(scope="module")
def ops(hip_device):
    from pixie_amd.unet import HipOps
    return HipOps(hip_device)


def per_tile_rel_l2(got, ref, tz, ty, tx):
    """worst rel-L2 over the (tz, ty, tx) blocks of a (C, D, H, W) output, all channels of a block together"""
    e = (np.asarray(got, np.float64) - np.asarray(ref, np.float64)) ** 2
    r = np.asarray(ref, np.float64) ** 2
    c, d, h, w = r.shape
    pz, py, px = (-d) % tz, (-h) % ty, (-w) % tx

    def blocks(a):
        a = np.pad(a.sum(0), ((0, pz), (0, py), (0, px)))
        return a.reshape((d + pz) // tz, tz, (h + py) // ty, ty, (w + px) // tx, tx).sum((1, 3, 5))

    return float(np.sqrt(blocks(e) / np.maximum(blocks(r), 1e-300)).max())


@functools.lru_cache(maxsize=1)     # the two paths of a row share the reference
def make_case(case, seed):
    """host tensors of a row and its float64 reference"""
    g = torch.Generator().manual_seed(seed)
    dims = tuple(case.dims)
    parts = [torch.randn((c,) + dims, generator=g) * (1.0 + 3.0 * i) for i, c in enumerate(case.cins)]
    parts[0] += 3.0
    cin = sum(case.cins)
    w = torch.randn((case.cout, cin) + (case.k,) * 3, generator=g) / np.sqrt(cin * case.k ** 3)
    bmag = 1.0 + torch.randn(case.cout, generator=g).abs()
    pro = (torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)) if case.pro != "none" else None
    affine = (torch.randn(dims, generator=g), torch.randn(dims, generator=g)) if case.pro == "channel+spatial" else None
    ref = ref_conv(parts, w, torch.zeros(case.cout), case.stride, case.up != "none", pro, affine, case.act, None)
    if case.out_size is not None:
        ref = ref[:, :case.out_size[0], :case.out_size[1], :case.out_size[2]]
    skip = None
    if case.skip:
        xs = [torch.randn((c,) + dims, generator=g) * (3.0 if i else 0.2) + (0.5 if i == 0 else 0.0) for i, c in enumerate(case.skip)]
        ws = torch.randn((case.cout, sum(case.skip), 1, 1, 1), generator=g) / np.sqrt(sum(case.skip))
        bs = torch.randn(case.cout, generator=g)
        ref = ref + ref_conv(xs, ws, bs)
        skip = (xs, ws, bs)
    residual = torch.randn(ref.shape, generator=g) if case.res else None
    if case.res:
        ref = ref + residual.double()
    # the bias (magnitude 1 + |N(0,1)|) takes the sign of its channel's mean, so that no channel's sum cancels: see the docstring
    mean = ref.reshape(case.cout, -1).mean(1)
    b = (torch.where(mean < 0, -bmag.double(), bmag.double())).float()
    ref = ref + b.double()[:, None, None, None]
    return parts, w, b, pro, affine, residual, skip, ref


PARAMS = [pytest.param(c, p, id=f"{c.id}-{p}") for c in VARIANT_CASES for p in runs(c)]


@pytest.mark.parametrize("case,precision", PARAMS)
def test_conv_variant(ops, case, precision):
    parts, w, b, pro, affine, residual, skip, ref = make_case(case, 1000 + VARIANT_CASES.index(case))
    dev = ops.device
    to = lambda t: t.to(dev) if t is not None else None
    dparts = [to(p) for p in parts]
    kw = dict(stride=case.stride, upsample=case.up != "none", pro=tuple(map(to, pro)) if pro else None,
              affine=tuple(map(to, affine)) if affine else None, act=case.act, residual=to(residual))
    if case.out_size is not None:
        kw["out_size"] = tuple(case.out_size)
    refn = ref.numpy()
    desc, oshape = operator_desc(precision, case.cins, case.cout, case.dims, case.k, stride=case.stride, upsample=case.up != "none",
                                 prologue=case.pro, residual=case.res, out_size=case.out_size, skip_cins=case.skip,
                                 subpixel=case.up == "sub-pixel", split_k=case.split_k)
    geo = tile_geometry(desc)
    assert geo is not None and tuple(oshape) == tuple(ref.shape)
    m = 2 if case.up == "sub-pixel" else 1       # sub-pixel tiles are given in stored voxels: each covers twice the extent of output
    tile = (m * geo["TZ"], m * geo["TY"], m * geo["TX"])
    tag = f"{case.id} {precision} <{case.k},{geo['MB']},{geo['NB']}> x{geo['slices']} tile {geo['TZ']}x{geo['TY']}x{geo['TX']} tiles {geo['tiles_z']}x{geo['tiles_y']}x{geo['tiles_x']}"

    def check(out, what):
        assert tuple(out.shape) == tuple(ref.shape)
        o = out.cpu().numpy()
        whole, worst = rel_l2(o, refn), per_tile_rel_l2(o, refn, *tile)
        print(f"{tag} {what}: rel-L2 whole {whole:.3e}, worst tile {worst:.3e}")
        assert whole < TOL[precision], (what, whole)
        assert worst < PER_TILE_TOL[precision], (what, worst)

    if precision == "f32":
        wp = ops.pack_conv(to(w))
        out = ops.conv(dparts, wp, to(b), case.cout, case.k, **kw)
        out2 = ops.conv(dparts, wp, to(b), case.cout, case.k, **kw)
        torch.cuda.synchronize()
        check(out, "exact")
        assert torch.equal(out, out2)
        return

    sub = case.up == "sub-pixel"
    kw["w16"] = ops.pack_conv_subpixel(to(w)) if sub else ops.pack_conv16(to(w))
    if sub:
        kw["subpixel"] = True
    if pro is not None:   # host bound on |prologue(x)|, deliberately loose by 3x: any valid bound must work
        kw["in_bound"] = 3.0 * float(_prologue_cpu(parts, pro, affine, case.act).abs().max())
    else:
        kw["in_amax"] = _amax_slots(ops, dparts)
    if skip is not None:
        dxs = [to(x) for x in skip[0]]
        kw["skip"] = dict(parts=dxs, w16=ops.pack_conv16(to(skip[1])), bias=to(skip[2]), amax=_amax_slots(ops, dxs))
    split = geo["slices"] > 1
    old = ops.split_k
    try:
        ops.split_k = case.split_k
        out = ops.conv(dparts, None, to(b), case.cout, case.k, **kw)
        out2 = ops.conv(dparts, None, to(b), case.cout, case.k, **kw)
        ops.split_k = case.split_k and not split          # the unsplit launch: the reference of a split one, and the one with statistics
        slot = torch.zeros(1, dtype=torch.int32, device=dev)
        uns, sums = ops.conv(dparts, None, to(b), case.cout, case.k, out_amax=slot, **kw)
    finally:
        ops.split_k = old
    torch.cuda.synchronize()
    check(out, "split" if split else "unsplit")
    assert torch.equal(out, out2)
    if split:
        check(uns, "unsplit")
        between = rel_l2(out.cpu().numpy(), uns.cpu().numpy())
        print(f"{tag}: split against unsplit {between:.3e}")
        assert between < 1e-6, between
    else:
        assert torch.equal(out, uns)      # asking for statistics does not change the output
    # epilogue statistics of the unsplit launch: against a separate pass over the written tensor, and against float64
    assert sums is not None and tuple(sums.shape) == (case.cout, 2)
    slot2 = torch.zeros(1, dtype=torch.int32, device=dev)
    again = ops.channel_stats(uns, slot2)
    assert rel_l2(sums.cpu().numpy(), again.cpu().numpy()) < 1e-6
    assert int(slot.item()) == int(slot2.item())   # same float bits
    assert abs(float(slot.view(torch.float32).item()) - float(uns.abs().max())) == 0.0
    r64 = ref.reshape(case.cout, -1)
    s = sums.cpu()
    e1 = float(((s[:, 0] - r64.sum(1)).abs() / r64.sum(1).abs().clamp_min(1e-300)).max())
    e2 = float(((s[:, 1] - (r64 * r64).sum(1)).abs() / (r64 * r64).sum(1)).max())
    print(f"{tag}: epilogue sums against float64: sum {e1:.2e}, sum of squares {e2:.2e} (worst channel, relative)")
    assert torch.allclose(s[:, 0], r64.sum(1), rtol=1e-5, atol=1e-3) and torch.allclose(s[:, 1], (r64 * r64).sum(1), rtol=1e-5)
