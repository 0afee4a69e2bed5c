"""CPU check of pixie_amd/csrc/conv_plan.h, the convolution launch planner as pure functions: g++ compiles the header alone (it
needs no HIP) into a small stand-alone program with -fsanitize=address,undefined, the program plans every row of
tests/golden/conv_plan_table.json from its SHAPE and FLAGS columns as plain integers (exact_v1 false), and its answers are compared
with the recorded columns by the rule of tests/test_conv_plan_table.py: exact for the descriptors pixie_conv3d_forward accepts; for
one it refuses, the recorded answer or "does not take this path".  The pair form's LDS bytes, which the table does not record, are
compared for every accepted row with what the PIXIE_DIAG library answers through pixie_conv_tile_geometry(desc, NULL) (a host
function: no device needed), so no rule is restated here."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "pixie_amd", "csrc", "conv_plan.h")
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_conv_plan_table as table      # noqa: E402
from pixie_amd import _lib                # noqa: E402
from test_conv_plan_table import NOT_THIS_PATH      # noqa: E402

# One line of 18 integers per row on stdin (SHAPE, then FLAGS); one line of answers per row on stdout, each what the entry point of
# include/pixie_hip.h named beside it answers from the same plan:
#   variant slices | geometry[10] or - | stats_floats | workspace_bytes (planned with workspace = true) | layout[6] or - | foldable | pair LDS
MAIN = r"""
#include <cstdio>
#include "%s"
using namespace pixie;
int main() {
    int v[18];
    for (;;) {
        for (int k = 0; k < 18; ++k)
            if (scanf("%%d", &v[k]) != 1) return k == 0 ? 0 : 2;
        ConvShape s;
        s.c0 = v[0]; s.c1 = v[1]; s.c_out = v[2]; s.in_d = v[3]; s.in_h = v[4]; s.in_w = v[5]; s.ksize = v[6]; s.stride = v[7]; s.upsample = v[8];
        s.out_d = v[9]; s.out_h = v[10]; s.out_w = v[11]; s.skip_c0 = v[12]; s.skip_c1 = v[13];
        s.w16 = v[14] != 0; s.subpixel = v[15] != 0; s.workspace = v[16] != 0; s.skip = v[17] != 0;
        const ConvPlan p = conv_plan(s);
        printf("%%d %%d |", conv_variant_number(p), p.f16x3() ? p.slices : 1);                  // pixie_conv_kernel_variant
        int32_t geo[10];
        if (conv_tile_geometry(p, geo)) for (int32_t g : geo) printf(" %%d", (int)g);           // pixie_conv_tile_geometry
        else printf(" -");
        printf(" | %%lld |", (long long)p.stats_floats);                                        // pixie_conv_stats_floats
        ConvShape w = s;
        w.workspace = true;
        printf(" %%lld |", (long long)conv_plan(w).workspace_bytes);                            // pixie_conv_workspace_bytes
        int64_t lay[6];
        if (conv_stats_layout(p, lay)) for (int64_t l : lay) printf(" %%lld", (long long)l);    // pixie_conv_stats_layout
        else printf(" -");
        printf(" | %%d | %%zu\n", p.skip_foldable ? 1 : 0, conv_pair_lds_bytes(p, s.skip));     // pixie_conv_skip_foldable; the launch form
    }
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_plan")
    src = d / "conv_plan_main.cpp"
    src.write_text(MAIN % HEADER)
    out = d / "conv_plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(out), str(src)])
    return str(out)


def numbers(part):
    return None if part.strip() == "-" else [int(w) for w in part.split()]


def test_the_header_plans_every_row_of_the_recorded_table(exe):
    with open(table.OUT) as f:
        doc = json.load(f)
    assert tuple(doc["columns"]) == table.COLUMNS
    rows = [dict(zip(table.COLUMNS, rec)) for rec in doc["rows"]]
    n_acc = sum(r["accepted"] for r in rows)
    assert len(rows) > 1000 and n_acc > 700      # the table is whole
    text = "".join(" ".join(str(int(r[c])) for c in table.SHAPE + table.FLAGS) + "\n" for r in rows)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", f"exit status {run.returncode}, the sanitizers said:\n{run.stderr}"
    lines = run.stdout.splitlines()
    assert len(lines) == len(rows)               # no row is skipped

    lib = _lib.load(diag=True)
    keep = C.c_int(0)                            # the launch-form switch: the plan's choice while the rows are asked, then as it was
    before = int(lib.pixie_conv_kernel_variant(None, C.byref(keep)))
    wrong, changed = [], 0
    try:
        for row, line in zip(rows, lines):
            head, geo, floats, ws, lay, fold, pair = line.split("|")
            variant, slices = numbers(head)
            now = {"variant": variant, "slices": slices, "geometry": numbers(geo), "stats_floats_asked": int(floats), "stats_floats": int(floats),
                   "workspace_bytes": int(ws), "layout": numbers(lay), "foldable": int(fold)}
            assert set(now) == set(table.ANSWERS[:-1])
            what = f"{[row[c] for c in table.SHAPE + table.FLAGS]} accepted={row['accepted']}"
            moved = False
            for k in table.ANSWERS[:-1]:
                if now[k] == row[k]:
                    continue
                if not row["accepted"] and now[k] == NOT_THIS_PATH[k]:
                    moved = True
                    continue
                wrong.append(f"{k}: recorded {row[k]}, the header {now[k]}  <- {what}")
            changed += moved
            if row["accepted"]:
                d = table.descriptor(row)
                lib_pair = int(lib.pixie_conv_tile_geometry(C.byref(d), None))
                if int(pair) != lib_pair:
                    wrong.append(f"pair-form LDS bytes: the library {lib_pair}, the header {int(pair)}  <- {what}")
    finally:
        keep = C.c_int(before)
        lib.pixie_conv_kernel_variant(None, C.byref(keep))
    print(f"{len(rows)} rows, {n_acc} accepted; refused rows that answer 'does not take this path' where the table recorded otherwise: "
          f"{changed} of {len(rows) - n_acc}; rows in the pair form: {sum(int(l.split('|')[6]) > 0 for l in lines)}")
    assert not wrong, f"{len(wrong)} answers differ:\n" + "\n".join(wrong[:20])
