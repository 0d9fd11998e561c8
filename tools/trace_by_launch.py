"""Per-launch-shape totals of a rocprofv3 --kernel-trace csv: kernels aggregated by (name, grid size), so that launches of
the same GEMM template at different shapes (environment transfers, matvec, gauge steps) are told apart.
usage: trace_by_launch.py kernel_trace.csv [--last 0.5] [--top 30]"""
import csv
import sys

path = sys.argv[1]
last = float(sys.argv[sys.argv.index("--last") + 1]) if "--last" in sys.argv else 1.0
top = int(sys.argv[sys.argv.index("--top") + 1]) if "--top" in sys.argv else 30
rows = []
with open(path) as f:
    for r in csv.DictReader(f):
        grid = "x".join(str(r.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0][-60:], grid))
rows.sort()
t0, t1 = rows[0][0], max(r[1] for r in rows)
lo = t1 - (t1 - t0) * last
rows = [r for r in rows if r[0] >= lo]
total = sum(e - s for s, e, _, _ in rows)
agg = {}
for s, e, n, g in rows:
    a = agg.setdefault((n, g), [0, 0])
    a[0] += 1
    a[1] += e - s
print(f"kernels {len(rows)}, summed kernel time {total / 1e6:.2f} ms")
for (n, g), (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:top]:
    print(f"  {t / 1e6:9.2f} ms {100 * t / total:5.1f} %  {c:6d} x {t / c / 1e3:8.2f} us  grid {g:>16}  {n}")
