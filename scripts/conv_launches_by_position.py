#!/usr/bin/env python
"""Conv launches of a `rocprofv3 --kernel-trace` database (rocpd sqlite) of bench.py, by kernel, grid and position inside a step.

Every pass over the two networks issues the same launches in the same order, so launch i of a (kernel, grid) class is position
i mod (launches per pass) of pass i div (launches per pass).  `passes` is the number of passes in the trace (bench.py --steps 20
--warmup 5 makes 30 over the pair of networks); 0 takes the greatest common divisor of the classes' launch counts, which counts the
two networks of a pair apart where they issue the same launches.  Prints avg / min / max us per position over the last `keep` passes (default 25: the timed steps and the warm-up
of `--steps 20 --warmup 5`) and the class's total per pass.
usage: conv_launches_by_position.py <results.db> [keep] [passes]"""
import math
import sqlite3
import sys
from collections import defaultdict

con = sqlite3.connect(sys.argv[1])
keep = int(sys.argv[2]) if len(sys.argv) > 2 else 25
cols = [d[0] for d in con.execute("select * from kernels limit 0").description]
start = next(c for c in ("start", "start_time", "start_timestamp", "begin") if c in cols)
rows = con.execute(f"select name, grid_x, grid_y, grid_z, duration from kernels where name like '%conv3d_%' order by {start}").fetchall()
by = defaultdict(list)
for name, gx, gy, gz, dur in rows:
    by[(name.split("(")[0], f"{gx}x{gy}x{gz}")].append(dur / 1e3)     # the kernels view is in nanoseconds
passes = int(sys.argv[3]) if len(sys.argv) > 3 else 0
if passes == 0:
    for v in by.values():
        passes = math.gcd(passes, len(v))
assert all(len(v) % passes == 0 for v in by.values()), "a class's launch count is no multiple of the number of passes"
print(f"{len(rows)} conv launches, {passes} network-pair passes")
for key, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    per = len(v) // passes
    last = v[(passes - min(keep, passes)) * per:]
    pos = [last[p::per] for p in range(per)]
    print(f"{key}: {per} launches per step; avg/min/max us over the last {min(keep, passes)} steps by position; total per step {sum(sum(p) / len(p) for p in pos):.1f} us")
    for i, p in enumerate(pos):
        print(f"  pos {i:3d}: {sum(p) / len(p):9.1f} {min(p):9.1f} {max(p):9.1f}")
