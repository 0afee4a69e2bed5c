"""CPU check of pixie_amd/csrc/hashmlp_plan.h, the pure-host policy of the 64-wide hash-grid MLP's training pass (layer shapes, the
slabs of the weight gradient, the byte layout of the saved activations and the scratch): g++ compiles it alone (it needs no HIP)
into a small stand-alone program with -fsanitize=address,undefined.  One case per line on stdin; the program prints the plan, which
is held to the restatement of the documented formula in tests/test_hashmlp_backward_capi.py and to the conditions the launch loop
of field_query_backward.hip relies on: the slabs it launches never exceed the slabs the scratch was sized for, every tile has a
slab, and every layer's partials fit their region."""
import itertools
import os
import subprocess

import pytest

import test_hashmlp_backward_capi as capi                  # its descriptors, parameter list and restatement of the formula: not written again

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pixie_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "%(csrc)s/hashmlp_plan.h"
using namespace pixie::hmp;

struct Desc { int n_levels, features_per_level, n_frequencies, n_extra, n_hidden, out_dim; long long table_rows; };

// n_levels features_per_level n_frequencies n_extra n_hidden out_dim table_rows n
int main() {
    Desc m;
    long long n;
    while (scanf("%%d %%d %%d %%d %%d %%d %%lld %%lld", &m.n_levels, &m.features_per_level, &m.n_frequencies, &m.n_extra, &m.n_hidden, &m.out_dim,
                 &m.table_rows, &n) == 8) {
        const ScratchLayout L = scratch_layout(m, (int64_t)n);
        printf("%%lld %%lld %%lld %%lld %%lld %%lld %%d", (long long)saved_bytes(m, (int64_t)n), (long long)L.total, (long long)L.dz, (long long)L.dxg,
               (long long)L.part, (long long)L.acc, pixie::hg::input_width(m));
        for (int i = 0; i <= m.n_hidden; ++i) {
            const int O = layer_out(m, i), K = layer_in(m, i);
            printf(" | %%d %%d %%d %%lld %%d", O, K, slab_count((int64_t)n, O, K), (long long)chunks_per_slab((int64_t)n, O, K), launched_slabs((int64_t)n, O, K));
        }
        printf("\n");
    }
    return 0;
}
"""

SHAPES = [kw for mark in capi.test_train_bytes_is_the_documented_formula.pytestmark if mark.args[0] == "kw" for kw in mark.args[1]]
SHAPES += [dict(n_hidden=h, out_dim=o) for h, o in itertools.product((1, 2, 3, 4), (1, 3, 63, 64, 65, 768))]
NS = [0, 1, 63, 64, 65, 200, 16383, 16384, 16385, 196608, 1 << 24]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(shape index, n): the program's line}, from one run under the sanitizers"""
    tmp = tmp_path_factory.mktemp("hashmlp_plan")
    src, exe = tmp / "hashmlp_plan_main.cpp", str(tmp / "hashmlp_plan_asan")
    src.write_text(MAIN % {"csrc": CSRC})
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(src), "-o", exe])
    cases = list(itertools.product(range(len(SHAPES)), NS))
    lines = []
    for s, n in cases:
        d = capi.desc(**SHAPES[s])
        lines.append(f"{d.n_levels} {d.features_per_level} {d.n_frequencies} {d.n_extra} {d.n_hidden} {d.out_dim} {d.table_rows} {n}")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-4000:]
    out = run.stdout.splitlines()
    assert len(out) == len(cases)
    return dict(zip(cases, out))


def parse(line):
    head, *layers = line.split(" | ")
    saved, total, dz, dxg, part, acc, width = (int(v) for v in head.split())
    return dict(saved=saved, total=total, dz=dz, dxg=dxg, part=part, acc=acc, width=width,
                layers=[dict(zip(("O", "K", "count", "chunks", "slabs"), (int(v) for v in l.split()))) for l in layers])


@pytest.mark.parametrize("s", range(len(SHAPES)), ids=lambda s: "-".join(f"{k}{v}" for k, v in SHAPES[s].items()) or "default")
def test_plan_holds_on_every_case(plans, s):
    d = capi.desc(**SHAPES[s])
    F = d.features_per_level if d.n_levels else 0
    for n in NS:
        p = parse(plans[(s, n)])
        # (a) the documented byte counts
        assert (p["saved"], p["total"]) == capi.documented_bytes(d, n), (n, p)
        assert len(p["layers"]) == d.n_hidden + 1 and p["layers"][0]["K"] == p["width"] and p["layers"][-1]["O"] == d.out_dim
        # (b) the launch loop's slabs against the slabs the scratch was sized for
        tiles = -(-n // 64)
        for l in p["layers"]:
            assert 1 <= l["slabs"] <= l["count"], (n, l)
            assert l["chunks"] >= 1 and l["chunks"] * l["slabs"] >= tiles, (n, l)
        # (c) the regions in order: header | dZ | dX of the grid | partials | accumulators
        sizes = [256, 4 * 64 * d.n_hidden * n, 4 * d.n_levels * F * n, max(4 * l["count"] * (l["O"] * l["K"] + l["O"]) for l in p["layers"]),
                 8 * d.table_rows * F]
        offsets = [0, p["dz"], p["dxg"], p["part"], p["acc"], p["total"]]
        assert all(o % 256 == 0 for o in offsets), (n, offsets)
        assert all(offsets[i] + sizes[i] <= offsets[i + 1] for i in range(5)), (n, offsets, sizes)
        # (d) what the launch loop writes for every layer fits the region of the partials
        for l in p["layers"]:
            assert 4 * l["slabs"] * (l["O"] * l["K"] + l["O"]) <= p["acc"] - p["part"], (n, l)
