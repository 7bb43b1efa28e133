#!/usr/bin/env python3
"""Per-chunk timeline of the align passes from a rocprofv3 --kernel-trace CSV of bench.py:
start / end of seed_lookup_kernel, simple_align_kernel, align_kernel<128> and <256> of every chunk
(ms from the first pass 0), the lag of <128>(c+1)'s start behind <128>(c)'s end (negative: it
started inside c's run) and where pass 0 / the simple pass of c+1 end relative to <128>(c)'s end.
   python3 tools/trace_chunks.py <run_kernel_trace.csv>"""
import csv
import sys

# (name prefixes: the align kernels carry their LV row capacity as a third template argument since round 17)
KERNELS = {"seed_lookup_kernel": "p0", "simple_align_kernel": "simple", "align_kernel<128, false": "k128",
           "align_kernel<256, false": "k256"}
rows = {v: [] for v in KERNELS.values()}
queues = {}
for r in csv.DictReader(open(sys.argv[1])):
    for name, key in KERNELS.items():
        if name in r["Kernel_Name"]:
            rows[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
            queues.setdefault(key, set()).add(r["Queue_Id"])
for v in rows.values():
    v.sort()
n = len(rows["k128"])
t0 = rows["p0"][0][0]
ms = lambda t: (t - t0) / 1e6
print("hardware queues:", {k: sorted(v) for k, v in queues.items()})
print("chunk  p0[start end]  simple[start end]  <128>[start end dur]  <256>[start end]  lag128  p0(c+1)-end128(c)  simple(c+1)-end128(c)")
lags = []
for c in range(n):
    f = lambda k: rows[k][c] if c < len(rows[k]) else None
    p0, si, k1, k2 = f("p0"), f("simple"), f("k128"), f("k256")
    cell = lambda x: f"{ms(x[0]):8.2f} {ms(x[1]):8.2f}" if x else "       -        -"
    line = f"{c:3d}  {cell(p0)}  {cell(si)}  {cell(k1)} {(k1[1] - k1[0]) / 1e6:6.2f}  {cell(k2)}"
    if c + 1 < n:
        nx, e = rows["k128"][c + 1], k1[1]
        lag = (nx[0] - e) / 1e6
        lags.append(lag)
        line += f"  {lag:7.2f}  {(rows['p0'][c + 1][1] - e) / 1e6:7.2f}"
        if c + 1 < len(rows["simple"]):
            line += f"  {(rows['simple'][c + 1][1] - e) / 1e6:7.2f}"
    print(line)
if n > 1:
    span = (rows["k128"][-1][1] - rows["k128"][0][1]) / 1e6 / (n - 1)
    print(f"<128> end-to-end period {span:.2f} ms per chunk; mean <128> duration "
          f"{sum(e - s for s, e in rows['k128']) / 1e6 / n:.2f} ms; mean lag {sum(lags) / len(lags):.2f} ms")
