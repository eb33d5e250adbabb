#!/usr/bin/env python3
"""Timeline of one step from a rocprofv3 rocpd .db: every kernel between two
launches of a marker kernel, with start and end in us from the first.

  ktimeline.py <rocpd.db> [marker substring, default csr_fwd_wide] [steps back, default 2]

The window runs from 30 us before the chosen marker launch to 30 us before
the next one, so kernels that start next to the marker on another stream
(the bottom MLP) fall into the same step."""
import re
import sqlite3
import sys

path = sys.argv[1]
marker = sys.argv[2] if len(sys.argv) > 2 else "csr_fwd_wide"
back = int(sys.argv[3]) if len(sys.argv) > 3 else 2
cur = sqlite3.connect(path).cursor()
t = [r[0] for r in cur.execute(
    "SELECT name FROM sqlite_master WHERE type='table' AND name LIKE 'rocpd_kernel_dispatch%'")][0]
u = t[len("rocpd_kernel_dispatch_"):]
cols = [r[1] for r in cur.execute(f"PRAGMA table_info({t})")]
lane = next((c for c in ("stream_id", "queue_id") if c in cols), "0")
rows = list(cur.execute(f"""
SELECT k.start, k.end, k.{lane}, ks.display_name
FROM rocpd_kernel_dispatch_{u} k
JOIN rocpd_info_kernel_symbol_{u} ks ON k.kernel_id = ks.id
ORDER BY k.start"""))
marks = [r[0] for r in rows if marker in r[3]]
assert len(marks) > back, f"only {len(marks)} launches of {marker}"
lo, hi = marks[-back - 1] - 30_000, marks[-back] - 30_000
step = [r for r in rows if lo <= r[0] < hi]
t0 = step[0][0]
print(f"# {len(step)} kernels, {(max(r[1] for r in step) - t0) / 1e3:.1f} us "
      f"from first start to last end; columns: start us, end us, us, {lane}, name")
for start, end, ln, name in step:
    name = re.sub(r"\s+", " ", name)[:100]
    print(f"{(start - t0) / 1e3:9.1f} {(end - t0) / 1e3:9.1f} {(end - start) / 1e3:8.1f} {ln!s:>4} {name}")
