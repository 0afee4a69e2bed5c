"""The conv launcher's answers, descriptor by descriptor, against the table recorded before it was rebuilt around one launch plan
(CPU only: pure host functions of the PIXIE_DIAG build; tests/golden/make_conv_plan_table.py wrote tests/golden/conv_plan_table.json).

For every descriptor pixie_conv3d_forward accepts (column `accepted`), pixie_conv_kernel_variant, pixie_conv_tile_geometry,
pixie_conv_stats_floats (statistics asked for or not), pixie_conv_workspace_bytes, pixie_conv_stats_layout and
pixie_conv_skip_foldable answer exactly what they answered then.  For a descriptor it refuses, a query may answer as it did, or
"does not take this path": 0 from the int64 queries and the variant, 1 (refused) from the geometry and the layout."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_conv_plan_table as table      # noqa: E402
from pixie_amd import _lib                # noqa: E402

NOT_THIS_PATH = {"variant": 0, "slices": 1, "geometry": None, "stats_floats_asked": 0, "stats_floats": 0, "workspace_bytes": 0,
                 "layout": None, "foldable": 0}


def test_every_query_answers_as_the_recorded_table():
    with open(table.OUT) as f:
        doc = json.load(f)
    assert tuple(doc["columns"]) == table.COLUMNS
    lib = _lib.load(diag=True)
    names = table.ANSWERS[:-1]
    wrong, changed, n_acc = [], 0, 0
    for rec in doc["rows"]:
        row = dict(zip(table.COLUMNS, rec))
        now = dict(zip(names, table.answers(lib, row)))
        n_acc += row["accepted"]
        moved = False
        for k in names:
            if now[k] == row[k]:
                continue
            if not row["accepted"] and now[k] == NOT_THIS_PATH[k]:
                moved = True
                continue
            wrong.append(f"{k}: recorded {row[k]}, now {now[k]}  <- {[row[c] for c in table.SHAPE + table.FLAGS]} accepted={row['accepted']}")
        changed += moved
    print(f"{len(doc['rows'])} rows, {n_acc} accepted; refused rows that now answer 'does not take this path' where they answered "
          f"otherwise before: {changed} of {len(doc['rows']) - n_acc}")
    assert len(doc["rows"]) > 1000 and n_acc > 700      # the table is whole
    assert not wrong, f"{len(wrong)} answers differ from the recorded table:\n" + "\n".join(wrong[:20])
