#!/usr/bin/env python3
"""Table of an alternating A/B of bench.py lines: <dir>/<wl>_<build>_<run>.json for builds parent and new.
   python3 tools/ab_table.py <dir> <c2|c3> <runs>"""
import json
import sys

o, wl, runs = sys.argv[1], sys.argv[2], int(sys.argv[3])
for v in ("parent", "new"):
    ds = [json.loads(open(f"{o}/{wl}_{v}_{i}.json").readline()) for i in range(1, runs + 1)]
    print(v.ljust(7), "M reads/s", [round(d["value"] / 1e6, 2) for d in ds], "kernel_busy_ms_per_step",
          [round(d["roofline"]["kernel_busy_ms_per_step"], 2) for d in ds])
