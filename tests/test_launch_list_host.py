"""CPU check of pixie_amd/csrc/launch_list.h, the launch list of a forward pass and merge_pair(), as pure functions: g++ compiles
the header alone (it needs no HIP) into a small stand-alone program with -fsanitize=address,undefined.  The program builds pairs of
hand-made lists, merges them and prints one line per emitted launch; the expectations are stated here.

A hand-made launch is written  <section><kernel><grid x>[y<grid y>][z<grid z>][l<LDS / 64>][b<block / 64>][!]  -- section f (full
resolution) or i (inner), kernel a letter, the numbers one digit each (defaults: grid y 1, grid z 3, LDS 64 bytes, block 256), `!` =
the kernel has NO grouped twin; its one argument is a number unique to the launch (1000 * list + position).  The program answers,
per emitted launch,  <list or g>:<kernel>:<grid x>x<grid z>:<arguments>  where a grouped launch (list `g`) names the twin (upper
case), has grid z doubled and carries both argument sets; a launch off the defaults also prints  :y<grid y>l<LDS>b<block>."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "pixie_amd", "csrc", "launch_list.h")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "%s"
using namespace pixie;
static char kernels[26], twins[26];
static LaunchList parse(const char* text, int which) {
    LaunchList l;
    int pos = 0;
    for (const char* p = text; *p && *p != '/'; ) {
        if (*p == ' ' || *p == '-') { ++p; continue; }
        LaunchRec r;
        r.section = *p++ == 'i' ? SEC_INNER : SEC_FULLRES;
        const int k = *p++ - 'a';
        r.kernel = &kernels[k];
        r.grid[0] = (uint32_t)(*p++ - '0');
        r.grid[2] = 3;
        r.block[0] = 256;
        r.lds = 64;
        r.twin = &twins[k];
        for (; *p && *p != ' ' && *p != '/'; ++p) {
            if (*p == '!') r.twin = nullptr;
            else if (*p == 'y') r.grid[1] = (uint32_t)(*++p - '0');
            else if (*p == 'z') r.grid[2] = (uint32_t)(*++p - '0');
            else if (*p == 'l') r.lds = 64u * (uint32_t)(*++p - '0');
            else if (*p == 'b') r.block[0] = 64u * (uint32_t)(*++p - '0');
            else exit(7);
        }
        const int64_t arg = 1000 * which + pos++;
        r.args.resize(sizeof arg);
        std::memcpy(r.args.data(), &arg, sizeof arg);
        r.offs.push_back(0);
        r.arg_stride = 16;          // as if the widest parameter were 16-byte aligned: the second set starts at the stride, not the size
        l.recs.push_back(r);
    }
    return l;
}
int main(int argc, char** argv) {
    for (int c = 1; c < argc; ++c) {
        const char* slash = std::strchr(argv[c], '/');
        if (!slash) return 2;
        const LaunchList a = parse(argv[c], 0), b = parse(slash + 1, 1);
        int grouped = -1;
        const std::vector<LaunchRec> m = merge_pair(a, b, &grouped);
        int seen = 0;
        for (const LaunchRec& r : m) {
            const bool g = r.net < 0;
            const char* base = g ? twins : kernels;
            const int k = (int)(static_cast<const char*>(r.kernel) - base);
            if (k < 0 || k >= 26 || r.offs.size() != 1 || r.offs[0] != 0 || r.block[1] != 1 || r.block[2] != 1) return 3;
            if (r.args.size() != (g ? 32u : 8u)) return 4;
            int64_t v0 = 0, v1 = 0;
            std::memcpy(&v0, r.args.data(), 8);
            if (g) std::memcpy(&v1, r.args.data() + 16, 8);
            if (g) printf("g:%%c:%%ux%%u:%%lld+%%lld", 'A' + k, r.grid[0], r.grid[2], (long long)v0, (long long)v1);
            else printf("%%d:%%c:%%ux%%u:%%lld", r.net, 'a' + k, r.grid[0], r.grid[2], (long long)v0);
            if (r.grid[1] != 1 || r.lds != 64 || r.block[0] != 256) printf(":y%%ul%%ub%%u", r.grid[1], r.lds, r.block[0]);
            printf(" ");
            seen += g;
        }
        if (seen != grouped) return 5;
        // group = false: every launch of both lists, none grouped
        int none = -1;
        if (merge_pair(a, b, &none, false).size() != a.recs.size() + b.recs.size() || none != 0) return 6;
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_list")
    src = d / "launch_list_main.cpp"
    src.write_text(MAIN % HEADER)
    out = d / "launch_list_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(out), str(src)])
    return str(out)


def merge(exe, *cases):
    run = subprocess.run([exe, *cases], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit status {run.returncode}, the sanitizers said:\n{run.stderr}"
    lines = [line.split() for line in run.stdout.splitlines()]
    assert len(lines) == len(cases)
    return lines if len(cases) > 1 else lines[0]


def test_section_order_and_grouping(exe):
    # encoder 0, encoder 1, the inner sections zipped (both positions match: grouped), decoder 0, decoder 1
    got = merge(exe, "fa1 fb1 - ic2 id2 - fe1 / fa1 fb1 - ic2 id2 - fe1")
    assert got == ["0:a:1x3:0", "0:b:1x3:1", "1:a:1x3:1000", "1:b:1x3:1001",
                   "g:C:2x6:2+1002", "g:D:2x6:3+1003",
                   "0:e:1x3:4", "1:e:1x3:1004"]


def test_grouping_needs_the_same_kernel_grid_and_a_twin(exe):
    other_kernel, other_grid, no_twin, twin_on_one_side = merge(
        exe, "fa1 ic2 ix2 fe1 / fa1 ic2 iy2 fe1", "fa1 ic2 id2 fe1 / fa1 ic2 id3 fe1", "fa1 ic2! id2 fe1 / fa1 ic2! id2 fe1", "fa1 ic2 fe1 / fa1 ic2! fe1")
    # a pair that does not match goes out as its two launches, list 0's first; the matching neighbours are still grouped
    assert other_kernel == ["0:a:1x3:0", "1:a:1x3:1000", "g:C:2x6:1+1001", "0:x:2x3:2", "1:y:2x3:1002", "0:e:1x3:3", "1:e:1x3:1003"]
    assert other_grid == ["0:a:1x3:0", "1:a:1x3:1000", "g:C:2x6:1+1001", "0:d:2x3:2", "1:d:3x3:1002", "0:e:1x3:3", "1:e:1x3:1003"]
    assert no_twin == ["0:a:1x3:0", "1:a:1x3:1000", "0:c:2x3:1", "1:c:2x3:1001", "g:D:2x6:2+1002", "0:e:1x3:3", "1:e:1x3:1003"]
    assert twin_on_one_side == ["0:a:1x3:0", "1:a:1x3:1000", "0:c:2x3:1", "1:c:2x3:1001", "0:e:1x3:2", "1:e:1x3:1002"]


def test_grouping_needs_the_same_lds_block_and_every_grid_dimension(exe):
    """One kernel, one grid x, a twin on both sides: a stride-2 and a stride-1 3^3 conv with the same output tile count, c_out and slices
    are that (conv_plan.h sizes the LDS tile from (T - 1) stride + ksize), and in lists of different length they can meet at one
    position.  Grouped, network 1's workgroups would run with network 0's LDS size.  Each pair below differs in ONE launch property
    and must go out as its two launches, each with its own; the neighbour that matches in all of them is still grouped."""
    lds, block, grid_y, grid_z, all_same = merge(
        exe, "ic2l2 id2 / ic2l3 id2", "ic2b4 id2 / ic2b8 id2", "ic2y2 id2 / ic2y4 id2", "ic2z2 id2 / ic2z4 id2", "ic2y2z2l3b8 / ic2y2z2l3b8")
    assert lds == ["0:c:2x3:0:y1l128b256", "1:c:2x3:1000:y1l192b256", "g:D:2x6:1+1001"]
    assert block == ["0:c:2x3:0", "1:c:2x3:1000:y1l64b512", "g:D:2x6:1+1001"]
    assert grid_y == ["0:c:2x3:0:y2l64b256", "1:c:2x3:1000:y4l64b256", "g:D:2x6:1+1001"]
    assert grid_z == ["0:c:2x2:0", "1:c:2x4:1000", "g:D:2x6:1+1001"]
    # the grouped launch keeps the pair's grid x and y, block and LDS; only grid z doubles
    assert all_same == ["g:C:2x4:0+1000:y2l192b512"]
    # lists of different length shift the positions: where the same kernel meets itself the two differ in LDS only, and stay apart
    shifted = merge(exe, "fa1 ix1 ic2l2 ic2l3 id2 / fa1 ic2l2 ic2l3 id2 iy1")
    assert shifted == ["0:a:1x3:0", "1:a:1x3:1000", "0:x:1x3:1", "1:c:2x3:1001:y1l128b256", "0:c:2x3:2:y1l128b256", "1:c:2x3:1002:y1l192b256",
                       "0:c:2x3:3:y1l192b256", "1:d:2x3:1003", "0:d:2x3:4", "1:y:1x3:1004"]


def test_unequal_and_empty_sections(exe):
    longer, shorter, no_inner_1, no_inner_both, empty_list, both_empty = merge(
        exe, "fa1 ic2 id2 ie2 ff1 / fa1 ic2 ff1", "fa1 ic2 ff1 / fa1 ic2 id2 ie2 ff1", "fa1 ic2 id2 ff1 / fa1 fb1", "fa1 fb1 / fa1", "fa1 ic2 ff1 /", "/")
    # what the longer inner section has beyond the shorter follows the zipped part, before either decoder section
    assert longer == ["0:a:1x3:0", "1:a:1x3:1000", "g:C:2x6:1+1001", "0:d:2x3:2", "0:e:2x3:3", "0:f:1x3:4", "1:f:1x3:1002"]
    assert shorter == ["0:a:1x3:0", "1:a:1x3:1000", "g:C:2x6:1+1001", "1:d:2x3:1002", "1:e:2x3:1003", "0:f:1x3:2", "1:f:1x3:1004"]
    # a list without an inner section is all encoder section; nothing to group, nothing lost
    assert no_inner_1 == ["0:a:1x3:0", "1:a:1x3:1000", "1:b:1x3:1001", "0:c:2x3:1", "0:d:2x3:2", "0:f:1x3:3"]
    assert no_inner_both == ["0:a:1x3:0", "0:b:1x3:1", "1:a:1x3:1000"]
    assert empty_list == ["0:a:1x3:0", "0:c:2x3:1", "0:f:1x3:2"]
    assert both_empty == []


def test_each_list_keeps_its_order_and_every_launch_appears_once(exe):
    # full-resolution marks INSIDE the inner run (they do not occur in a U-Net walk) stay in place: the run is first to last inner mark
    cases = ["fa1 fb2 ic1 id2 fe3 if1 ig2! fh1 fi2 / fa1 fb3 ic1 id2 ie3 if1 ig2! fh1",
             "ia1 ib1 / fa1 ib1 ic1 fd1 fe1",
             "fa1 fb1 fc1 / ia1 ia1 ia1 ia1"]
    for case, got in zip(cases, merge(exe, *cases)):
        want = [[1000 * k + i for i in range(len(side.split()))] for k, side in enumerate(case.split("/"))]
        seen = [[], []]
        for item in got:
            net, _, _, args = item.split(":")
            if net == "g":
                a0, a1 = (int(v) for v in args.split("+"))
                seen[0].append(a0)
                seen[1].append(a1)
            else:
                seen[int(net)].append(int(args))
        assert seen == want, case
