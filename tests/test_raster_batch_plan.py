"""CPU check of pixie_amd/csrc/raster_batch_plan.h, the host function that partitions the views of a rasteriser batch into sort
groups: g++ compiles it alone (it needs no HIP) into a small program with -fsanitize=address,undefined, and its answers are compared
with the Python restatement below."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "pixie_amd", "csrc", "raster_batch_plan.h")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "%s"
// argv: capacity max_views count...   ->   "groups b0 b1 ..." or "error v"
int main(int argc, char** argv) {
    const uint64_t capacity = strtoull(argv[1], nullptr, 10);
    const int max_views = atoi(argv[2]);
    std::vector<uint64_t> counts;
    for (int i = 3; i < argc; ++i) counts.push_back(strtoull(argv[i], nullptr, 10));
    std::vector<int32_t> begin(counts.size() + 1, -7);
    const int64_t g = pixie::raster::plan_groups(counts.data(), (int)counts.size(), capacity, max_views, begin.data());
    if (g < 0) { printf("error %%lld\n", (long long)(-1 - g)); return 0; }
    printf("groups");
    for (int64_t k = 0; k <= g; ++k) printf(" %%d", begin[k]);
    printf("\n");
    return 0;
}
"""


def plan(counts, capacity, max_views):
    """Greedy over consecutive views: ("groups", boundaries) or ("error", first view that alone exceeds the capacity)."""
    for v, c in enumerate(counts):
        if c > capacity:
            return "error", [v]
    begin, total = [0], 0
    for v, c in enumerate(counts):
        if v > begin[-1] and (total + c > capacity or v - begin[-1] == max_views):
            begin.append(v)
            total = 0
        total += c
    return "groups", begin + [len(counts)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("raster_batch_plan")
    src = d / "plan_main.cpp"
    src.write_text(MAIN % HEADER)
    out = d / "plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(out), str(src)])
    return str(out)


def run(exe, counts, capacity, max_views=65535):
    words = subprocess.check_output([exe, str(capacity), str(max_views)] + [str(c) for c in counts], text=True).split()
    return words[0], [int(w) for w in words[1:]]


CASES = [
    ("all counts zero", [0, 0, 0, 0], 0, 65535, ("groups", [0, 4])),
    ("one view exactly at capacity", [100], 100, 65535, ("groups", [0, 1])),
    ("one view at capacity among others", [40, 100, 60, 40], 100, 65535, ("groups", [0, 1, 2, 4])),
    ("one view over capacity", [10, 20, 101, 500], 100, 65535, ("error", [2])),
    ("groups of 1, 2 and 3 views", [90, 50, 50, 30, 30, 40, 10], 100, 65535, ("groups", [0, 1, 3, 6, 7])),
    ("capacity >= the total", [5, 6, 7, 8], 26, 65535, ("groups", [0, 4])),
    ("capacity above the total", [5, 6, 7, 8], 1 << 40, 65535, ("groups", [0, 4])),
    ("1 view", [17], 1000, 65535, ("groups", [0, 1])),
    ("1 empty view", [0], 0, 65535, ("groups", [0, 1])),
    ("empty views join a full group", [100, 0, 0, 1], 100, 65535, ("groups", [0, 3, 4])),
    ("the view limit of the key bits", [1, 1, 1, 1, 1], 100, 2, ("groups", [0, 2, 4, 5])),
    ("counts near 2^32 do not wrap", [4294967295, 4294967295, 1], 4294967295, 65535, ("groups", [0, 1, 2, 3])),
]


@pytest.mark.parametrize("name,counts,capacity,max_views,want", CASES, ids=[c[0] for c in CASES])
def test_plan_matches_the_restatement(exe, name, counts, capacity, max_views, want):
    assert plan(counts, capacity, max_views) == want              # the restatement says what the case is meant to show
    assert run(exe, counts, capacity, max_views) == want


def test_plan_on_seeded_random_counts(exe):
    import random
    rng = random.Random(5)
    for _ in range(40):
        counts = [rng.choice([0, 0, rng.randrange(1, 50), rng.randrange(50, 400)]) for _ in range(rng.randrange(1, 12))]
        capacity, max_views = rng.randrange(1, 900), rng.choice([1, 2, 3, 65535])
        got = run(exe, counts, capacity, max_views)
        assert got == plan(counts, capacity, max_views), (counts, capacity, max_views)
        if got[0] == "groups":
            b = got[1]
            assert b[0] == 0 and b[-1] == len(counts) and all(x < y for x, y in zip(b, b[1:]))
            assert all(sum(counts[x:y]) <= capacity and y - x <= max_views for x, y in zip(b, b[1:]))
