#!/usr/bin/env python3
"""What duplicate marking of 1M aligned reads' sorted BAM costs: marked on the device, where the records lie,
against records downloaded, marked by the host model and compressed again.

bench.py's C2 workload (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99), ids r<i>.  Every
child process builds the world, aligns the reads and computes their CIGARs once on the GPU, then
times three legs that alternate in the process, warm medians of `--reps` after one warm-up of each:

  a   run_bam(sorted) + run_dupmark + run_bgzf + run_bai + bgzf() + bai(): wall time to both files' bytes in
      host memory, the mark kernels' ms (all passes and each pass, HIP events), the marked and group counts;
  b   the same chain without the mark call: the cost the marking adds is a - b;
  c   run_bam(sorted) + bam() (the records' download), snapgpu.bam_mark_duplicates on the host, then
      aligner.bgzf_compress of the marked bytes: the only way to a marked stream without the device pass.
      It builds no index, so it is the shorter of the host routes.

The score pass's effective rate is the bytes it has to move (every record's QUAL, its 36 fixed bytes, its two
starts, and the 12 bytes it writes) over its event time, beside the streaming-copy peak copy_peak_ms reports
for the records' bytes.  One child runs on 16 host threads (SNAPGPU_HOST_THREADS=16) and one on 2, a rank's
share of the host on an 8-GPU node.  The first child also checks that the device's records equal the host
model's.  There is no threshold: the report states what was measured.  It goes to --out, rewritten after
every child.

Every child runs under its own time limit and the first one that fails, faults or times out ends the
run: nothing is started on a GPU after a failure.

    python3 tools/dupmark_time.py --reps 7 --out profiles/r20/dupmark.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))

# bench.py WORKLOADS["c2"]
C2 = dict(genome_bases=46_709_983, n_contigs=1, families=200, reads=1_000_000)
CHILD_LIMIT_S = 420
PASSES = ("fields_and_score", "run_numbering", "best_per_group", "mark", "check")


def _stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def child(reps, n_reads, genome_bases):
    import snapgpu
    lib = snapgpu.lib()
    g = snapgpu.Genome.synthetic(genome_bases, seed=2121, n_contigs=C2["n_contigs"], n_repeat_families=C2["families"])
    idx = snapgpu.GenomeIndex.build(g, 20, 16, device=0)
    reads = snapgpu.Reads.synthetic(idx.genome_handle(), n_reads, seed=99)
    ids = [b"r%d" % i for i in range(reads.n)]
    al = snapgpu.BaseAligner(idx)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    dev.synchronize()
    pass_ms = lib.snapgpu_internal_dupmark_pass_ms
    pass_ms.restype, pass_ms.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    n_ref = C2["n_contigs"]

    def chain(mark):
        t = time.perf_counter()
        dev.run_bam(reads, ids=ids, sorted_output=True)
        if mark:
            dev.run_dupmark()
        dev.run_bgzf()
        dev.run_bai(0)
        z = dev.bgzf()
        bai = dev.bai()
        return (time.perf_counter() - t) * 1e3, z, bai

    def host():
        t = time.perf_counter()
        dev.run_bam(reads, ids=ids, sorted_output=True)
        raw = dev.bam()
        t1 = time.perf_counter()
        marked, n_marked, n_groups = snapgpu.bam_mark_duplicates(raw, n_ref)
        t2 = time.perf_counter()
        z = al.bgzf_compress(marked)
        t3 = time.perf_counter()
        return (t3 - t) * 1e3, (t1 - t) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, marked, (n_marked, n_groups), z

    chain(True)   # warm-ups
    want = dev.bam()
    counts = dev.dupmark_stats()
    chain(False)
    _, _, _, _, model, model_counts, _ = host()
    lengths = reads.lengths()
    score_bytes = int(lengths.sum()) + reads.n * (36 + 16 + 12)
    peak_ms = al.copy_peak_ms(len(want))
    a, b, c, down, mark, comp, kern, passes = [], [], [], [], [], [], [], []
    for _ in range(reps):
        ms, z, _ = chain(True)
        a.append(ms)
        kern.append(al.dupmark_ms()[0])
        p = (C.c_double * len(PASSES))()
        assert pass_ms(al._h, p) == 0
        passes.append(list(p))
        assert dev.dupmark_stats() == counts
        b.append(chain(False)[0])
        ms, dl, mk, cp, _, _, _ = host()
        c.append(ms)
        down.append(dl)
        mark.append(mk)
        comp.append(cp)
    score_ms = statistics.median(p[0] for p in passes)
    out = {"host_threads": snapgpu.host_threads(), "reads": reads.n, "record_bytes": len(want),
           "marked": counts[0], "groups": counts[1], "device_equals_model": want == model and counts == model_counts,
           "a_wall_ms": _stats(a), "b_wall_ms": _stats(b), "c_wall_ms": _stats(c),
           "c_records_download_ms": _stats(down), "c_host_mark_ms": _stats(mark), "c_device_compress_ms": _stats(comp),
           "a_mark_kernel_ms": _stats(kern),
           "a_pass_ms": {name: _stats([p[k] for p in passes]) for k, name in enumerate(PASSES)},
           "score_pass_bytes": score_bytes, "score_pass_gb_per_s": round(score_bytes / score_ms / 1e6, 1),
           "copy_peak_ms": round(peak_ms, 3), "copy_peak_gb_per_s": round(2 * len(want) / peak_ms / 1e6, 1)}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "dupmark.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be at least 3")
    if args.child:
        child(args.reps, args.reads, args.genome_bases)
        return 0

    report = {"tool": "tools/dupmark_time.py", "reps": args.reps, "reads": args.reads, "genome_bases": args.genome_bases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for threads in (16, 2):
        name = "threads_%d" % threads
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--reads", str(args.reads),
               "--genome-bases", str(args.genome_bases)]
        env = dict(os.environ, SNAPGPU_HOST_THREADS=str(threads))
        print(f"[{name}] ...", flush=True)
        failed = None
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S, env=env)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:
                failed = {"child": name, "returncode": p.returncode, "stderr": p.stderr[-2000:]}
        except subprocess.TimeoutExpired:
            failed = {"child": name, "returncode": "time limit"}
        if failed:
            report["stopped_at"] = failed
            save()
            print("STOPPED: " + json.dumps(failed), flush=True)
            return 1
        report[name] = json.loads(line[len("RESULT "):])
        save()
        print(f"[{name}] " + json.dumps(report[name]), flush=True)
    t16, t2 = report["threads_16"], report["threads_2"]
    for leg in "abc":
        report[f"{leg}_wall_median_ms_16_threads"] = t16[f"{leg}_wall_ms"]["median"]
        report[f"{leg}_wall_median_ms_2_threads"] = t2[f"{leg}_wall_ms"]["median"]
    save()
    print(f"a {t16['a_wall_ms']['median']} / {t2['a_wall_ms']['median']} ms, b {t16['b_wall_ms']['median']} / "
          f"{t2['b_wall_ms']['median']} ms, c {t16['c_wall_ms']['median']} / {t2['c_wall_ms']['median']} ms (16 / 2 host threads); "
          f"mark kernels {t16['a_mark_kernel_ms']['median']} ms, {t16['marked']} marked in {t16['groups']} groups; "
          f"equals model: {t16['device_equals_model']}", flush=True)
    return 0 if t16["device_equals_model"] and t2["device_equals_model"] else 2


if __name__ == "__main__":
    sys.exit(main())
