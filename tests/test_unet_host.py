"""CPU check of the two pure-host headers behind the U-Net handle, pixie_amd/csrc/unet_plan.h (the network as data) and
pixie_amd/csrc/workspace_arena.h (the first-fit free list that places every temporary of a pass): g++ compiles them alone (they need
no HIP) into one small stand-alone program with -fsanitize=address,undefined.

plan mode:  one configuration per line on stdin; the program prints the block lists, out_sp and the state_dict table, which are held
            to pixie_amd.unet_plan (build_plan, param_shapes with its order, is_norm_key) for the configurations of
            tests/test_unet_handle.py and a sweep over depth, attention levels, blocks per level, grid sizes (odd ones too) and the
            three projector kinds.
arena mode: a script of requests on stdin; the program prints every offset it hands out, the peak and the final free list, which are
            held to a plain Python model (sorted free ranges, lowest offset that fits, 256-byte granules).  Equal offsets for equal
            scripts is the property that lets a dry run size the real pass."""
import bisect
import itertools
import os
import random
import subprocess

import pytest

from pixie_amd.unet_plan import UNetConfig, build_plan, is_norm_key, param_shapes
from test_unet_handle import CONFIGS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pixie_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%(csrc)s/unet_plan.h"
#include "%(csrc)s/workspace_arena.h"
using namespace pixie::unet;

// feature_channels cond_dim model_channels num_res_blocks grid_size out_channels n_mult mult... n_attn attn...
static int plan_mode() {
    static const char* kinds[] = {"conv_in", "res", "down", "attn", "up"};
    for (;;) {
        Cfg c;
        int n = 0;
        if (scanf("%%d", &c.feature_channels) != 1) return 0;
        if (scanf("%%d %%d %%d %%d %%d %%d", &c.cond_dim, &c.model_channels, &c.num_res_blocks, &c.grid_size, &c.out_channels, &n) != 6) return 2;
        c.precision = 0;
        for (int i = 0, v; i < n; ++i) { if (scanf("%%d", &v) != 1) return 2; c.mult.push_back(v); }
        if (scanf("%%d", &n) != 1) return 2;
        for (int i = 0, v; i < n; ++i) { if (scanf("%%d", &v) != 1) return 2; c.attn.push_back(v); }
        const Plan p = build_plan(c);
        auto seq = [&](const char* part, const std::vector<Blk>& s) {
            printf("%%s", part);
            for (const Blk& b : s) printf(" | %%s %%s %%d %%d %%d", kinds[b.kind], b.prefix.c_str(), b.cin, b.cout, b.sp);
            printf("\n");
        };
        for (auto& s : p.in_blocks) seq("in", s);
        seq("middle", p.middle);
        for (auto& s : p.out_blocks) seq("out", s);
        printf("out_sp %%d\n", p.out_sp);
        for (const ParamSpec& q : param_table(c, p)) {
            printf("param %%s %%d %%lld :", q.key.c_str(), q.norm ? 1 : 0, (long long)q.numel);
            for (int64_t d : q.shape) printf(" %%lld", (long long)d);
            printf("\n");
        }
        printf("end\n");
    }
}

// a BYTES: alloc | r K: release the offset the K-th alloc returned | x OFFSET: release an offset as given
static int arena_mode(long long capacity) {
    Arena a;
    a.reset(nullptr, capacity);
    std::vector<int64_t> issued;
    char op;
    long long v;
    while (scanf(" %%c %%lld", &op, &v) == 2) {
        if (op == 'a') { issued.push_back(a.alloc(v)); printf("%%lld\n", (long long)issued.back()); }
        else if (op == 'r') { if (v < 0 || v >= (long long)issued.size()) return 2; a.release(issued[(size_t)v]); }
        else if (op == 'x') a.release(v);
        else return 2;
    }
    printf("peak %%lld\nfree", (long long)a.peak);
    for (auto& kv : a.free_) printf(" %%lld %%lld", (long long)kv.first, (long long)kv.second);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_mode();
    if (argc == 3 && !strcmp(argv[1], "arena")) return arena_mode(atoll(argv[2]));
    return 2;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("unet_host")
    src = d / "unet_host_main.cpp"
    src.write_text(MAIN % {"csrc": CSRC})
    out = d / "unet_host_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(out), str(src)])
    return str(out)


def run(exe, args, text):
    r = subprocess.run([exe] + args, input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"exit status {r.returncode}, the sanitizers said:\n{r.stderr}"
    return r.stdout.splitlines()


# ---------------------------------------------------------------- plan mode
def sweep():
    cfgs = list(CONFIGS.values())
    for mult, attn, nrb, grid, feat in itertools.product([(1,), (1, 2), (1, 2, 3), (1, 1, 2, 4)], [(), (1,), (2,), (1, 2, 4, 8)], [1, 2, 3],
                                                         [8, 9, 13, 16], [32, 16, 64]):      # feat = / < / > cond_dim: no, light, hidden-128 projector
        cfgs.append(UNetConfig(feat, 32, 32, nrb, mult, attn, grid, 3))
    return cfgs


def test_plan_and_state_dict_table_equal_the_python_plan(exe):
    cfgs = sweep()
    assert len(cfgs) == 4 + 4 * 4 * 3 * 4 * 3
    assert {(c.has_projector, c.projector_hidden) for c in cfgs} == {(False, None), (True, None), (True, 128)}
    text = "".join(f"{c.feature_channels} {c.cond_dim} {c.model_channels} {c.num_res_blocks} {c.grid_size} {c.out_channels} "
                   f"{len(c.channel_mult)} {' '.join(map(str, c.channel_mult))} {len(c.attention_resolutions)} "
                   f"{' '.join(map(str, c.attention_resolutions))}\n" for c in cfgs)
    lines = iter(run(exe, ["plan"], text))
    for cfg in cfgs:
        got = {"in": [], "middle": [], "out": []}
        params, out_sp = [], None
        for line in lines:
            if line == "end":
                break
            word = line.split()[0]
            if word == "out_sp":
                out_sp = int(line.split()[1])
            elif word == "param":
                head, shape = line.split(":")
                _, key, norm, numel = head.split()
                params.append((key, tuple(int(s) for s in shape.split()), int(norm), int(numel)))
            else:
                got[word].append([(b[0], b[1], int(b[2]), int(b[3]), int(b[4])) for b in (part.split() for part in line.split("|")[1:])])
        else:
            pytest.fail("the program's output ended inside a configuration")
        plan = build_plan(cfg)
        blocks = lambda seq: [(b.kind, b.prefix, b.cin, b.cout, b.sp) for b in seq]      # noqa: E731
        assert got["in"] == [blocks(s) for s in plan.input_blocks], cfg
        assert got["middle"] == [blocks(plan.middle)], cfg
        assert got["out"] == [blocks(s) for s in plan.output_blocks], cfg
        assert out_sp == plan.out_sp, cfg
        shapes = param_shapes(cfg)
        assert [(k, s) for k, s, _, _ in params] == [(k, tuple(s)) for k, s in shapes.items()], cfg      # order included
        for key, shape, norm, numel in params:
            assert bool(norm) == is_norm_key(key), (cfg, key)
            n = 1
            for s in shape:
                n *= s
            assert numel == n, (cfg, key)
    assert next(lines, None) is None


# ---------------------------------------------------------------- arena mode
ALIGN = 256
SIZES = [0, 1, 255, 256, 257]


class Model:
    """A sorted list of free [offset, size) ranges; the lowest offset that fits; release coalesces with both neighbours."""

    def __init__(self, capacity):
        self.free, self.used, self.peak = [[0, capacity]], {}, 0

    def alloc(self, nbytes):
        n = max((nbytes + ALIGN - 1) // ALIGN * ALIGN, ALIGN)
        for i, (off, size) in enumerate(self.free):
            if size >= n:
                if size == n:
                    del self.free[i]
                else:
                    self.free[i] = [off + n, size - n]
                self.used[off] = n
                self.peak = max(self.peak, off + n)
                return off
        return -1

    def release(self, off):
        n = self.used.pop(off, None)
        if n is None:
            return
        i = bisect.bisect_left(self.free, [off, 0])
        if i < len(self.free) and self.free[i][0] == off + n:
            n += self.free.pop(i)[1]
        if i > 0 and sum(self.free[i - 1]) == off:
            self.free[i - 1][1] += n
        else:
            self.free.insert(i, [off, n])


def script(seed, n_ops=2000):
    """alloc / release requests, then a release of everything still live.  Releases name an allocation by its number, mostly a live
    one, sometimes one released before (a no-op unless its offset is in use again: then it frees that one, for the model as well)."""
    rng = random.Random(seed)
    ops, n_alloc, live = [], 0, []
    for _ in range(n_ops):
        u = rng.random()
        if u < 0.55 or not live:
            ops.append(("a", rng.choice(SIZES) if rng.random() < 0.3 else rng.randint(1, 1 << 20)))
            live.append(n_alloc)
            n_alloc += 1
        elif u < 0.93:
            ops.append(("r", live.pop(rng.randrange(len(live)))))
        elif u < 0.96:
            ops.append(("r", rng.randrange(n_alloc)))
        else:
            ops.append(("x", rng.randrange(1 << 30) * ALIGN + rng.randint(1, ALIGN - 1)))      # not a multiple of 256: never issued
    return ops + [("r", k) for k in range(n_alloc)]


def replay(exe, ops, capacity):
    """Runs the script through the program and the model side by side; returns (offsets, number of refusals)."""
    out = run(exe, ["arena", str(capacity)], "".join(f"{op} {v}\n" for op, v in ops))
    offsets = [int(x) for x in out[:-2]]
    assert len(offsets) == sum(op == "a" for op, _ in ops)
    model, live, ends, k = Model(capacity), {}, [0], 0
    for op, v in ops:
        if op == "a":
            off = offsets[k]
            assert off == model.alloc(v), f"allocation {k} of {v} bytes"
            if off >= 0:
                n = max((v + ALIGN - 1) // ALIGN * ALIGN, ALIGN)
                assert off % ALIGN == 0 and off + n <= capacity
                assert all(off + n <= o or o + m <= off for o, m in live.items()), f"allocation {k} overlaps a live range"
                live[off] = n
                ends.append(off + n)
            k += 1
        else:
            off = offsets[v] if op == "r" else v
            live.pop(off, None)
            model.release(off)
    assert not live
    assert out[-2] == f"peak {max(ends)}" and max(ends) == model.peak
    assert out[-1] == f"free 0 {capacity}" and model.free == [[0, capacity]]      # everything released: one range again
    return offsets, sum(o < 0 for o in offsets)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_arena_places_as_the_model_does(exe, seed):
    ops = script(seed)
    big = 1 << 50      # the dry run's capacity
    offsets, refused = replay(exe, ops, big)
    assert refused == 0
    assert replay(exe, ops, big)[0] == offsets      # the same script, the same placement
    # a capacity the script does not fit in: exhaustion answers -1 and leaves the state usable (what follows still matches the model)
    tight = max(offsets) // 2 // ALIGN * ALIGN
    assert replay(exe, ops, tight)[1] >= 1
