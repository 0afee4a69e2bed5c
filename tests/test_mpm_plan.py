"""CPU check of pixie_amd/csrc/mpm_plan.h, the MPM solver's host decisions as pure functions (re-binning cadence, work-item size
hysteresis, scatter mode, fused kernel variant, crowded grid, BC motion, modifier order, BC sets, batched launch groups and the byte
layout of the batch tables): g++ compiles it alone (it needs no HIP) into a small program with -fsanitize=address,undefined, and its
answers are compared with the Python restatements below, written from the solver's code before the functions were extracted."""
import os
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "pixie_amd", "csrc", "mpm_plan.h")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "%s"
using namespace pixie;
static float f_of(const char* bits) { unsigned u = (unsigned)strtoul(bits, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }
static unsigned bits_of(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
    const std::string cmd = argv[1];
    char** a = argv + 2;
    if (cmd == "cadence") printf("%%d\n", next_resort_interval(atoi(a[0]), strtod(a[1], nullptr), strtoull(a[2], nullptr, 10), atoi(a[3])));
    else if (cmd == "half") printf("%%d\n", (int)half_items_wanted(atoi(a[0]) != 0, atol(a[1]), atol(a[2])));
    else if (cmd == "scatter") {   // user lo hi (float bits) -> contrast bits, mode
        const float c = mass_contrast_of(f_of(a[1]), f_of(a[2]));
        printf("%%08x %%d\n", bits_of(c), scatter_bits_for(atoi(a[0]), c));
    }
    else if (cmd == "scatter_at") printf("%%d\n", scatter_bits_for(atoi(a[0]), f_of(a[1])));
    else if (cmd == "fused") printf("%%d\n", (int)fused_variant(atoi(a[0]), atoi(a[1]), atoi(a[2]), atoi(a[3]), atoi(a[4])));
    else if (cmd == "crowded") printf("%%d\n", (int)grid_crowded(atol(a[0]), atoi(a[1])));
    else if (cmd == "advance") {   // time dt n { type start end p[3] v[3] }  (doubles as C99 hex)  ->  per BC: device point bits, host point
        const double time = strtod(a[0], nullptr), dt = strtod(a[1], nullptr);
        const int n = atoi(a[2]);
        a += 3;
        std::vector<pixie_bc_desc> bcs(n);
        std::vector<BCDev> dev;
        for (int k = 0; k < n; ++k, a += 9) {
            memset(&bcs[k], 0, sizeof bcs[k]);
            bcs[k].type = atoi(a[0]); bcs[k].start_time = strtod(a[1], nullptr); bcs[k].end_time = strtod(a[2], nullptr);
            for (int d = 0; d < 3; ++d) { bcs[k].point[d] = strtod(a[3 + d], nullptr); bcs[k].velocity[d] = strtod(a[6 + d], nullptr); }
            dev.push_back(to_dev(bcs[k]));
        }
        advance_bcs_state(time, bcs, dev, dt);
        for (int k = 0; k < n; ++k) {
            for (int d = 0; d < 3; ++d) printf("%%08x ", bits_of(dev[k].point[d]));
            for (int d = 0; d < 3; ++d) printf("%%a ", bcs[k].point[d]);
        }
        printf("\n");
    }
    else if (cmd == "pmods") {     // time(bits) all n { type start(bits) end(bits) }  ->  registration indices in launch order
        const float time = f_of(a[0]);
        const bool all = atoi(a[1]) != 0;
        const int n = atoi(a[2]);
        a += 3;
        std::vector<PModDev> pm(n);
        for (int k = 0; k < n; ++k, a += 3) {
            memset(&pm[k], 0, sizeof pm[k]);
            pm[k].type = atoi(a[0]); pm[k].start = f_of(a[1]); pm[k].end = f_of(a[2]); pm[k].rot_scale = (float)k;
        }
        for (const PModDev& m : active_pmods(pm, time, all)) printf("%%d ", (int)m.rot_scale);
        printf("\n");
    }
    else if (cmd == "bcset") {     // size first  ->  n, then the indices of the BCs in the set
        std::vector<BCDev> dev(atoi(a[0]));
        for (size_t k = 0; k < dev.size(); ++k) { memset(&dev[k], 0, sizeof dev[k]); dev[k].pad = (int)k; }
        const BCSet set = make_bcset(dev, (size_t)strtoull(a[1], nullptr, 10));
        printf("%%d", set.n);
        for (int k = 0; k < set.n; ++k) printf(" %%d", set.bc[k].pad);
        printf("\n");
    }
    else if (cmd == "xform") {     // 16 doubles: shift[3] scale mean[3] inv_rotation[9]  ->  17 float bit patterns in struct order
        double v[16];
        for (int k = 0; k < 16; ++k) v[k] = strtod(a[k], nullptr);
        const FrameXform X = make_frame_xform(v, v[3], v + 4, v + 7);
        unsigned w[17];
        static_assert(sizeof X == sizeof w, "FrameXform is 17 floats");
        memcpy(w, &X, sizeof w);
        for (unsigned u : w) printf("%%08x ", u);
        printf("\n");
    }
    else if (cmd == "groups") {    // ns { run g2p p2g cap pack fv n_items xcd }  ->  one line per launch
        const int ns = atoi(a[0]);
        a += 1;
        std::vector<BatchSceneKind> sc(ns);
        for (int s = 0; s < ns; ++s, a += 8)
            sc[s] = BatchSceneKind{atoi(a[0]) != 0, atoi(a[1]) != 0, atoi(a[2]) != 0, atoi(a[3]), atoi(a[4]) != 0, (FusedVariant)atoi(a[5]), atoi(a[6]), atoi(a[7]) != 0};
        std::vector<char> done(ns, 0);
        BatchGroup g;
        while (next_batch_group(sc.data(), ns, done.data(), &g)) {
            printf("%%d %%d %%d %%d %%d %%d %%ld :", (int)g.g2p, (int)g.p2g, (int)g.pack, g.item_cap, (int)g.fv, g.xcd_order, g.total);
            for (int k = 0; k < g.n; ++k) printf(" %%d", g.scene[k]);
            printf(" :");
            for (int k = 0; k <= g.n; ++k) printf(" %%d", g.first[k]);
            printf("\n");
        }
    }
    else if (cmd == "layout") {    // 6 record sizes, ns with_export with_splats { n_win n_bc moving }  ->  sp_off.. bc_off.. bc_stride.. ex spl total
        BatchTableSizes z{};
        size_t* zs[6] = {&z.scene, &z.step_params, &z.bc_head, &z.bc_dev, &z.export_rec, &z.splat_rec};
        for (int k = 0; k < 6; ++k) *zs[k] = (size_t)strtoull(a[k], nullptr, 10);
        const int ns = atoi(a[6]);
        const bool ex = atoi(a[7]) != 0, spl = atoi(a[8]) != 0;
        a += 9;
        std::vector<int> n_win(ns);
        std::vector<size_t> n_bc(ns);
        std::vector<char> moving(ns);
        for (int s = 0; s < ns; ++s, a += 3) { n_win[s] = atoi(a[0]); n_bc[s] = (size_t)atoi(a[1]); moving[s] = (char)atoi(a[2]); }
        BatchTableLayout L;
        batch_table_layout(z, ns, n_win.data(), n_bc.data(), moving.data(), ex, spl, &L);
        for (const std::vector<size_t>* v : {&L.sp_off, &L.bc_off, &L.bc_stride})
            for (size_t x : *v) printf("%%zu ", x);
        printf("%%zu %%zu %%zu\n", L.ex_off, L.spl_off, L.total);
    }
    else return 2;
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mpm_plan")
    src = d / "plan_main.cpp"
    src.write_text(MAIN % HEADER)
    out = d / "plan_main"
    # (-Wno-unknown-pragmas: mpm_math.h, which mpm_types.h takes MaterialScalars from, carries `#pragma unroll` for hipcc)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(out), str(src)])
    return str(out)


def run(exe, *args):
    return subprocess.check_output([exe] + [str(a) for a in args], text=True)


def ints(exe, *args):
    return [int(w) for w in run(exe, *args).split()]


def fbits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


# ---------------------------------------------------------------- cadence (rebin(): the body under `n_sorts > 0 && xref_valid`)
def cadence(k0, drift, slow, n):
    k = k0
    if drift > 0.0:
        k = int(min(4.0 * k, max(0.25 * k, k * 0.4 / drift)))
    else:
        k = 4 * k
    if slow > n // 1000:
        k = min(k, k0 // 2)
    return max(2, min(k, 1024))


N = 100_000
CADENCE = [(4, 0.0, 0, N, 16), (512, 0.0, 0, N, 1024), (4, 0.4, 0, N, 4), (37, 0.4, 0, N, 37), (1024, 0.4, 0, N, 1024), (8, 0.1, 0, N, 32),
           (8, 4.0, 0, N, 2), (4, 10.0, 0, N, 2), (64, 0.0, N // 1000 + 1, N, 32), (64, 0.0, N // 1000, N, 256), (2, 0.0, N, N, 2),
           (100, 0.05, 0, N, 400), (100, 1.0, 0, N, 40), (7, 0.3, 101, N, 3)]


@pytest.mark.parametrize("k,drift,slow,n,want", CADENCE)
def test_cadence(exe, k, drift, slow, n, want):
    assert cadence(k, drift, slow, n) == want
    assert ints(exe, "cadence", k, float(drift).hex(), slow, n) == [want]


def test_cadence_on_seeded_random_inputs(exe):
    import random
    rng = random.Random(3)
    for _ in range(40):
        k, drift = rng.randrange(2, 1025), rng.choice([0.0, rng.uniform(1e-4, 0.2), rng.uniform(0.2, 6.0)])
        n = rng.randrange(1, 2_000_000)
        slow = rng.choice([0, n // 1000, n // 1000 + 1, n])
        assert ints(exe, "cadence", k, float(drift).hex(), slow, n) == [cadence(k, drift, slow, n)], (k, drift, slow, n)


# ---------------------------------------------------------------- 128 / 256 work items: enter at <= 15 % more items, stay up to 25 %
@pytest.mark.parametrize("on,n128,n256,want", [(0, 1150, 1000, 1), (0, 1160, 1000, 0), (1, 1250, 1000, 1), (1, 1260, 1000, 0),
                                               (0, 1151, 1000, 0), (1, 1251, 1000, 0), (1, 1160, 1000, 1), (0, 0, 0, 1), (0, 916, 526, 0)])
def test_item_size_hysteresis(exe, on, n128, n256, want):
    assert int(n128 * 100 <= n256 * (125 if on else 115)) == want
    assert ints(exe, "half", on, n128, n256) == [want]


# ---------------------------------------------------------------- scatter mode
def test_scatter_mode(exe):
    above = np.nextafter(np.float32(32.0), np.float32(64.0))
    assert ints(exe, "scatter_at", 0, fbits(32.0)) == [32] and ints(exe, "scatter_at", 0, fbits(above)) == [64]
    assert ints(exe, "scatter_at", 64, fbits(1.0)) == [64] and ints(exe, "scatter_at", 32, fbits(1000.0)) == [32]
    # contrast = hi / lo in float32, through the same threshold
    for lo, hi in ((1.0, 32.0), (1.0, float(above)), (0.3, 9.6), (3e-7, 1e-5), (2.5, 2.5)):
        c = np.float32(hi) / np.float32(lo)
        assert run(exe, "scatter", 0, fbits(lo), fbits(hi)).split() == [fbits(c), str(64 if c > np.float32(32.0) else 32)]
    # the three guards: no positive mass seen (lo = the 0xffffffff fill is a NaN, or 0), hi < lo, hi not finite  ->  contrast 1
    for lo_bits, hi_bits in (("ffffffff", "00000000"), (fbits(0.0), fbits(5.0)), (fbits(2.0), fbits(1.0)), (fbits(1.0), fbits(np.inf)),
                             (fbits(1.0), fbits(3.0e38))):
        assert run(exe, "scatter", 0, lo_bits, hi_bits).split() == [fbits(1.0), "32"]


# ---------------------------------------------------------------- fused variant, crowded grid
def fused(wide, n_items, n_cus, occ, bits):
    if wide == 1 or (wide < 0 and n_items <= 3 * n_cus):
        return 1
    return 2 if occ >= 6 and bits != 32 else 0


def test_fused_variant(exe):
    cases = [(-1, 768, 256, 5, 32, 1), (-1, 769, 256, 5, 32, 0), (-1, 769, 256, 6, 64, 2), (-1, 769, 256, 6, 32, 0), (0, 10, 256, 5, 32, 0),
             (1, 100000, 256, 6, 64, 1), (0, 10, 256, 6, 64, 2), (0, 10, 256, 6, 32, 0), (-1, 768, 256, 6, 64, 1), (-1, 912, 304, 5, 64, 1)]
    for wide, n_items, n_cus, occ, bits, want in cases:
        assert fused(wide, n_items, n_cus, occ, bits) == want
        assert ints(exe, "fused", wide, n_items, n_cus, occ, bits) == [want]


def test_crowded_grid(exe):
    for n, cus, want in ((2048, 256, 0), (2049, 256, 1), (0, 256, 0), (520, 256, 0), (2600, 256, 1), (8 * 304 + 1, 304, 1), (3_000_000_000, 256, 1)):
        assert int(n > 8 * cus) == want
        assert ints(exe, "crowded", n, cus) == [want]


# ---------------------------------------------------------------- moving cuboids
def advance(time, dt, bcs):
    """bcs: (type, start, end, point, velocity) in doubles; -> per BC (device point as float32, host point as float)"""
    out = []
    for typ, start, end, p, v in bcs:
        dev_p, dev_v = np.array(p, np.float64).astype(np.float32), np.array(v, np.float64).astype(np.float32)
        host = list(p)
        if typ == 1 and float(np.float32(start)) <= time < float(np.float32(end)):
            dev_p = (dev_p.astype(np.float64) + dt * dev_v.astype(np.float64)).astype(np.float32)
            host = [float(q) for q in dev_p]
        out.append((dev_p, host))
    return out


def test_advance_bcs_state(exe):
    start, end = 0.1, 0.30000000000000004          # neither is a float32: the window is compared after rounding to float
    f_start, f_end = float(np.float32(start)), float(np.float32(end))
    assert f_start > start and f_end > end
    p, v = [1.0, 0.7, 0.55], [0.0, 0.2, 0.1]
    dt = 1e-4
    still = (0, start, end, [0.1, 0.2, 0.3], [1.0, 1.0, 1.0])      # a surface: untouched
    for time, moves in ((start, False), (np.nextafter(f_start, 0.0), False), (f_start, True), (0.2, True), (end, True),
                        (np.nextafter(f_end, 0.0), True), (f_end, False), (0.5, False)):
        bcs = [(1, start, end, p, v), still, (2, start, end, p, v)]
        want = advance(float(time), dt, bcs)
        assert (want[0][1] != p) == moves and want[1][1] == still[3] and want[2][1] == p
        args = []
        for typ, s, e, pp, vv in bcs:
            args += [typ, float(s).hex(), float(e).hex()] + [float(q).hex() for q in pp + vv]
        words = run(exe, "advance", float(time).hex(), float(dt).hex(), len(bcs), *args).split()
        for k, (dev_p, host) in enumerate(want):
            assert words[6 * k:6 * k + 3] == [fbits(q) for q in dev_p], (time, k)
            assert [float.fromhex(w) for w in words[6 * k + 3:6 * k + 6]] == host, (time, k)


# ---------------------------------------------------------------- modifiers: impulses first, stable otherwise, float window
def pmods(mods, time, all_):
    t = np.float32(time)
    order = []
    for impulse_pass in (True, False):
        for k, (typ, start, end) in enumerate(mods):
            if (typ == 0) != impulse_pass:
                continue
            if not all_ and not (t >= np.float32(start) and t < np.float32(end)):
                continue
            order.append(k)
    return order


def test_active_pmods(exe):
    mods = [(1, 0.0, 1.0), (0, 0.001, 0.0015), (2, 0.0, 0.001), (0, 0.0, 1.0), (1, 0.002, 0.003), (0, 0.001, 0.001)]
    assert pmods(mods, 0.0, True) == [1, 3, 5, 0, 2, 4]
    assert pmods(mods, 0.001, False) == [1, 3, 0]
    for time in (0.0, 0.001, float(np.nextafter(np.float32(0.001), np.float32(0.0))), 0.0015, 0.0025, 5.0):
        for all_ in (0, 1):
            args = []
            for typ, s, e in mods:
                args += [typ, fbits(s), fbits(e)]
            assert ints(exe, "pmods", fbits(time), all_, len(mods), *args) == pmods(mods, time, all_), (time, all_)
    assert ints(exe, "pmods", fbits(0.0), 1, 0) == []


# ---------------------------------------------------------------- BC sets of one launch
@pytest.mark.parametrize("size", [0, 16, 17, 33])
@pytest.mark.parametrize("first", [0, 16, 32, 40])
def test_make_bcset(exe, size, first):
    want = list(range(min(first, size), size))[:16]
    assert ints(exe, "bcset", size, first) == [len(want)] + want


def test_make_frame_xform(exe):
    shift, scale, mean = [0.1, -0.2, 0.30000000000000004], 1.7, [1.0 / 3.0, 2.0, -5.5]
    rot = [0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6]
    want = [np.float32(x) for x in shift] + [np.float32(1.0 / scale)] + [np.float32(x) for x in mean] + [np.float32(1.0 / (scale * scale))] + \
           [np.float32(x) for x in rot]
    assert run(exe, "xform", *[float(x).hex() for x in shift + [scale] + mean + rot]).split() == [fbits(x) for x in want]


# ---------------------------------------------------------------- batched launch groups (the loop of batch_issue_particle)
def groups(sc):
    """sc: dicts run g2p p2g cap pack fv n_items xcd  ->  [(g2p, p2g, pack, cap, fv, xcd, total, scenes, first)]"""
    done, out = [False] * len(sc), []
    for s0, k0 in enumerate(sc):
        if done[s0] or not k0["run"]:
            continue
        scenes, first, total, xcd = [], [], 0, 1
        for s in range(s0, len(sc)):
            k = sc[s]
            if done[s] or not k["run"] or k["g2p"] != k0["g2p"] or k["p2g"] != k0["p2g"]:
                continue
            if k["cap"] != k0["cap"] or (k0["p2g"] and k["pack"] != k0["pack"]):
                continue
            if k0["g2p"] and k0["p2g"] and k["fv"] != k0["fv"]:
                continue
            done[s] = True
            scenes.append(s)
            first.append(total)
            total += k["n_items"]
            if not k["xcd"]:
                xcd = 0
        out.append((int(k0["g2p"]), int(k0["p2g"]), int(k0["pack"]), k0["cap"], k0["fv"], xcd, total, scenes, first + [total]))
    return out


def run_groups(exe, sc):
    args = []
    for k in sc:
        args += [int(k["run"]), int(k["g2p"]), int(k["p2g"]), k["cap"], int(k["pack"]), k["fv"], k["n_items"], int(k["xcd"])]
    out = []
    for line in run(exe, "groups", len(sc), *args).splitlines():
        head, scenes, first = [[int(w) for w in part.split()] for part in line.split(":")]
        out.append(tuple(head) + (scenes, first))
    return out


def kind(**kw):
    k = dict(run=True, g2p=True, p2g=True, cap=256, pack=True, fv=0, n_items=10, xcd=True)
    k.update(kw)
    return k


def test_groups_of_one_kind(exe):
    sc = [kind(n_items=100 + 7 * s) for s in range(32)]
    got = run_groups(exe, sc)
    first = [sum(k["n_items"] for k in sc[:s]) for s in range(33)]
    assert got == [(1, 1, 1, 256, 0, 1, first[-1], list(range(32)), first)] == groups(sc)


GROUP_CASES = {
    "capacity splits": ([kind(cap=256), kind(cap=128), kind(cap=256)], [[0, 2], [1]]),
    "scatter mode splits a fused launch": ([kind(), kind(pack=False), kind()], [[0, 2], [1]]),
    "scatter mode is shared under g2p-only": ([kind(p2g=False), kind(p2g=False, pack=False)], [[0, 1]]),
    "scatter mode splits p2g-only": ([kind(g2p=False), kind(g2p=False, pack=False)], [[0], [1]]),
    "fused variant splits a fused launch": ([kind(fv=1), kind(fv=0), kind(fv=2, pack=False), kind(fv=1)], [[0, 3], [1], [2]]),
    "fused variant is shared under p2g-only": ([kind(g2p=False, fv=1), kind(g2p=False, fv=0)], [[0, 1]]),
    "fused variant is shared under g2p-only": ([kind(p2g=False, fv=1), kind(p2g=False, fv=2)], [[0, 1]]),
    "launch kinds split": ([kind(), kind(p2g=False), kind(g2p=False), kind(), kind(p2g=False)], [[0, 3], [1, 4], [2]]),
    "a scene that does not run, in the middle": ([kind(), kind(run=False, n_items=0), kind()], [[0, 2]]),
    "the first scene does not run": ([kind(run=False), kind(), kind()], [[1, 2]]),
    "nothing runs": ([kind(run=False), kind(run=False)], []),
    "one scene": ([kind(n_items=1)], [[0]]),
}


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_groups(exe, name):
    sc, scenes = GROUP_CASES[name]
    got = run_groups(exe, sc)
    assert [g[7] for g in got] == scenes
    assert got == groups(sc)


def test_group_xcd_order(exe):
    sc = [kind(), kind(xcd=False), kind(), kind(cap=128)]
    got = run_groups(exe, sc)
    assert got == groups(sc)
    assert [(g[7], g[5]) for g in got] == [([0, 1, 2], 0), ([3], 1)]


def test_groups_on_seeded_random_scenes(exe):
    import random
    rng = random.Random(11)
    for _ in range(30):
        sc = [kind(run=rng.random() < 0.8, g2p=(kd := rng.choice([(1, 1), (1, 1), (1, 0), (0, 1)]))[0] == 1, p2g=kd[1] == 1, cap=rng.choice([128, 256]),
                   pack=rng.random() < 0.5, fv=rng.randrange(3), n_items=rng.randrange(1, 5000), xcd=rng.random() < 0.8) for _ in range(rng.randrange(1, 33))]
        got = run_groups(exe, sc)
        assert got == groups(sc)
        assert sorted(s for g in got for s in g[7]) == [s for s, k in enumerate(sc) if k["run"]]      # every running scene exactly once


# ---------------------------------------------------------------- byte layout of the batch tables (batch_upload)
SIZES = dict(scene=1200, step_params=100, bc_head=4, bc_dev=76, export_rec=120, splat_rec=24)   # the records' sizes are parameters


def align_up(v, a):
    return (v + a - 1) // a * a


def layout(z, scenes, with_export, with_splats):
    """scenes: (n_win, n_bc, moving)  ->  sp_off, bc_off, bc_stride, ex_off, spl_off, total"""
    ns = len(scenes)
    off = align_up(z["scene"] * ns, 256)
    sp_off, bc_off, bc_stride = [], [], []
    for n_win, _, _ in scenes:
        sp_off.append(off)
        off = align_up(off + (n_win + 1) * z["step_params"], 16)
    for n_win, n_bc, moving in scenes:
        rec = align_up(z["bc_head"] + n_bc * z["bc_dev"], 16)
        bc_stride.append(rec if moving else 0)
        bc_off.append(off)
        off += rec * n_win if moving else rec
    ex_off = spl_off = 0
    if with_export:
        ex_off = off = align_up(off, 16)
        off += ns * z["export_rec"]
    if with_splats:
        spl_off = off = align_up(off, 16)
        off += ns * z["splat_rec"]
    return sp_off, bc_off, bc_stride, ex_off, spl_off, off


def run_layout(exe, z, scenes, with_export, with_splats):
    args = [z[k] for k in ("scene", "step_params", "bc_head", "bc_dev", "export_rec", "splat_rec")] + [len(scenes), int(with_export), int(with_splats)]
    for sc in scenes:
        args += [sc[0], sc[1], int(sc[2])]
    w = ints(exe, "layout", *args)
    ns = len(scenes)
    return w[:ns], w[ns:2 * ns], w[2 * ns:3 * ns], w[3 * ns], w[3 * ns + 1], w[3 * ns + 2]


def layout_scenes(ns, n_win, moving):
    return [(n_win if s % 3 != 2 else max(n_win - 5, 0), (0, 1, 16, 3)[s % 4], moving and s % 2 == 0) for s in range(ns)]


@pytest.mark.parametrize("ns", [1, 32])
@pytest.mark.parametrize("n_win", [0, 1024])
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("with_export,with_splats", [(False, False), (True, False), (True, True)])
def test_layout(exe, ns, n_win, moving, with_export, with_splats):
    z = SIZES
    scenes = layout_scenes(ns, n_win, moving)
    got = run_layout(exe, z, scenes, with_export, with_splats)
    assert got == layout(z, scenes, with_export, with_splats)
    sp_off, bc_off, bc_stride, ex_off, spl_off, total = got
    regions = [(0, z["scene"] * ns, 1)]                                        # (start, bytes, alignment)
    for s, (nw, n_bc, mv) in enumerate(scenes):      # every scene's StepParams table, then every scene's BC records
        regions.append((sp_off[s], (nw + 1) * z["step_params"], 256 if s == 0 else 16))
    for s, (nw, n_bc, mv) in enumerate(scenes):
        rec = z["bc_head"] + n_bc * z["bc_dev"]
        assert bc_stride[s] == (align_up(rec, 16) if mv else 0)
        regions.append((bc_off[s], (nw - 1) * bc_stride[s] + rec if mv and nw else (0 if mv else rec), 16))
    assert (ex_off != 0) == with_export and (spl_off != 0) == with_splats
    if with_export:
        regions.append((ex_off, ns * z["export_rec"], 16))
    if with_splats:
        regions.append((spl_off, ns * z["splat_rec"], 16))
    end = 0
    for start, size, align in regions:           # in table order: inside [0, total), disjoint, aligned
        assert start >= end and start % align == 0 and start + size <= total, (start, size, align, end, total)
        end = start + size
