"""How the simple pass (simple_align_kernel) routes a bench workload's reads: the records it writes, those of
them written by its one-read path (nSimpleWide: what the four-reads-per-wave path hands on), the reads it
bails, and -- from the records -- the share of the one-element / one-scored reads with score <= 7, the limit
of the quad path's narrow LV pass.  One JSON line.
  python tools/simple_wide_share.py [--workload c2|c3] [--reads N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))
import numpy as np  # noqa: E402
import snapgpu  # noqa: E402

SHAPES = {"c2": dict(genome_bases=46_709_983, contigs=1, families=200),
          "c3": dict(genome_bases=3_100_000_000, contigs=25, families=2000)}   # bench.py WORKLOADS

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=sorted(SHAPES), default="c2")
ap.add_argument("--reads", type=int, default=1_000_000)
args = ap.parse_args()
wl = SHAPES[args.workload]
g = snapgpu.Genome.synthetic(wl["genome_bases"], seed=2121, n_contigs=wl["contigs"], n_repeat_families=wl["families"])
reads = snapgpu.Reads.synthetic(g, args.reads, seed=99)
idx = snapgpu.GenomeIndex.build(g, 20, 16)
del g
al = snapgpu.BaseAligner(idx, device=0)
res = al.AlignReads(reads)
t = al.timing()
one = (res["nElements"] == 1) & (res["nLocationsScored"] == 1)
out = {"workload": args.workload, "reads": args.reads,
       "nSimpleReads": t["nSimpleReads"], "nSimpleBailed": t["nSimpleBailed"], "nSimpleWide": t["nSimpleWide"],
       "wide_share_of_simple_reads": t["nSimpleWide"] / max(1, t["nSimpleReads"]),
       "one_element_one_scored": int(one.sum()),
       "of_them_score_le_7": int((one & (res["score"] <= 7)).sum()),
       "score_histogram_0_to_16": np.bincount(res["score"][one].clip(0, 16), minlength=17).tolist()}
out["share_score_le_7"] = out["of_them_score_le_7"] / max(1, out["one_element_one_scored"])
print(json.dumps(out))
