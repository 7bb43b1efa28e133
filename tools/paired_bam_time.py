#!/usr/bin/env python3
"""Time of the BAM records of 500k aligned read pairs: the host encoder against the device chain.

bench.py --full's paired workload on C2 (chr21-sized synthetic genome, 500k 2 x 101 pairs, seed 7),
the ids those pairs get when they are written as FASTQ.  Every child process builds the world and
aligns the pairs once on the GPU (snapgpu_paired_align_batch), then times, on the same results:

  H  the host path: CIGARs of both ends through the existing batch call (snapgpu_cigar_batch per
     end), their rows interleaved into the encoder's 2n (a numpy copy), then
     snapgpu_bam_format_pairs into a fresh uninitialised buffer -- ms of each part and of all;
  D  the device chain over the resident batch: snapgpu_paired_cigar_resident +
     snapgpu_paired_bam_resident + snapgpu_paired_bam_download -- wall ms from the first call to the
     records in host memory, and the CIGAR, encoder-kernel (HIP events) and download parts;
  S  the same chain with snapgpu_paired_bam_resident_sorted (coordinate order); the sort step's share
     is S's encoder-kernel ms less D's, both between HIP events.

All at 16 host threads (one child alternates H, D and S `--reps` times after a warm-up of each) and
at 2, a rank's share of the host on an 8-GPU node (a child of its own: the budget is read once per
process).  D's bytes must equal H's, and S's the stable reorder of H's records by
snapgpu_bam_pair_sort_keys (SHA-256).  No threshold: the report states D and S against H.

Every child runs under its own time limit and the first one that fails, faults or times out ends
the run: nothing is started on a GPU after a failure.

    python3 tools/paired_bam_time.py --reps 7 --out profiles/r24/paired_bam.json
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))

# bench.py WORKLOADS["c2"] and its paired leg
C2 = dict(genome_bases=46_709_983, n_contigs=1, families=200, pairs=500_000, seed=7, read_length=101)
CHILD_LIMIT_S = 420


def _stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def child(reps, n_pairs, genome_bases):
    import numpy as np
    import snapgpu
    g = snapgpu.Genome.synthetic(genome_bases, seed=2121, n_contigs=C2["n_contigs"], n_repeat_families=C2["families"])
    idx = snapgpu.GenomeIndex.build(g, 20, 16, device=0)
    s0, s1 = snapgpu.Reads.synthetic_pairs(idx.genome_handle(), n_pairs, seed=C2["seed"], read_length=C2["read_length"])
    with tempfile.TemporaryDirectory() as tmp:   # the batches with ids: the FASTQ form of the same pairs
        reads = []
        for e, s in enumerate((s0, s1)):
            path = os.path.join(tmp, f"p_{e + 1}.fq")
            s.write_fastq(path)
            reads.append(snapgpu.Reads.from_fastq(path))
    r0, r1 = reads
    pa = snapgpu.PairedAligner(idx, device=0)
    base = snapgpu.BaseAligner(idx, maxHitsToConsider=16000, maxK=15, maxSeedsToUse=8, extraSearchDepth=2)
    res = pa.align(r0, r1)
    out = {"host_threads": snapgpu.host_threads(), "pairs": r0.n,
           "mapped_ends": int((res["status"] != snapgpu.NotFound).sum())}

    lib = snapgpu.lib()
    loc, dr = snapgpu._pair_cigar_inputs(res)
    cap = int(sum(int(np.ctypeslib.as_array(r._p.contents.idLengths, shape=(r.n,)).sum()) + 2 * int(r._p.contents.totalBytes)
                  for r in (r0, r1))) + 2 * r0.n * 512
    used = C.c_uint64()

    carry = C.c_int32()

    def host():
        t0 = time.perf_counter()
        ends = [base.Cigars(r, loc[e::2], dr[e::2]) for e, r in enumerate((r0, r1))]   # snapgpu_cigar_batch per end
        t1 = time.perf_counter()
        cig = snapgpu.Cigars.empty(2 * r0.n)   # the 2n rows the encoder takes: row 2q + e
        for e, k in enumerate(ends):
            cig.editDistance[e::2], cig.nOps[e::2], cig.ops[e::2] = k.editDistance, k.nOps, k.ops
        t2 = time.perf_counter()
        buf = np.empty(cap, dtype=np.uint8)
        rc = lib.snapgpu_bam_format_pairs(idx._h, r0._p, r1._p, res.ctypes.data, cig.editDistance.ctypes.data,
                                          cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ", 0, C.byref(carry),
                                          buf.ctypes.data, cap, C.byref(used))
        t3 = time.perf_counter()
        assert rc == 0, snapgpu.last_error()
        return ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), buf[:used.value], carry.value

    def device(sorted_output):
        t0 = time.perf_counter()
        rc = lib.snapgpu_paired_cigar_resident(pa._h, res.ctypes.data, 0)
        assert rc == 0, snapgpu.last_error()
        fn = lib.snapgpu_paired_bam_resident_sorted if sorted_output else lib.snapgpu_paired_bam_resident
        rc = fn(pa._h, r0._p, r1._p, b"FASTQ", 0)
        assert rc == 0, snapgpu.last_error()
        lib.snapgpu_paired_bam_download(pa._h, None, 0, C.byref(used), C.byref(carry))
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        rc = lib.snapgpu_paired_bam_download(pa._h, buf.ctypes.data, used.value, C.byref(used), C.byref(carry))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, snapgpu.last_error()
        kernel_ms, download_ms = pa.bam_ms()
        return ms, (pa.sam_ms()[0], kernel_ms, download_ms), hashlib.sha256(buf[:used.value]).hexdigest(), used.value, carry.value

    _, records, host_carry = host()
    device(False)
    device(True)   # warm-up of all legs (buffers grown, staging pinned)
    # what S must give: H's records in the stable order of their sort keys
    starts = np.zeros(2 * r0.n + 1, dtype=np.int64)
    starts[1:] = np.cumsum(snapgpu.bam_pair_record_lengths(idx, r0, r1, res, _cigars(snapgpu, base, r0, r1, loc, dr)))
    order = np.argsort(snapgpu.bam_pair_sort_keys(idx, res), kind="stable")
    want_sorted = hashlib.sha256(b"".join(records[starts[j]:starts[j + 1]].tobytes() for j in order)).hexdigest()
    hp, d, s, parts, sparts = [], [], [], [], []
    digests = {"H": set(), "D": set(), "S": set()}
    nbytes = 0
    for _ in range(reps):
        p, buf, hc = host()
        nbytes = len(buf)
        hp.append(p)
        digests["H"].add(hashlib.sha256(buf).hexdigest())
        for sorted_output, wall, part, key in ((False, d, parts, "D"), (True, s, sparts, "S")):
            ms, p, h, nb, dc = device(sorted_output)
            assert nb == nbytes and dc == hc == host_carry
            wall.append(ms)
            part.append(p)
            digests[key].add(h)
    out.update({
        "H_cigar_calls_ms": _stats([p[0] for p in hp]), "H_cigar_rows_interleave_ms": _stats([p[1] for p in hp]),
        "H_format_ms": _stats([p[2] for p in hp]), "H_wall_ms": _stats([sum(p) for p in hp]),
        "H_wall_without_interleave_ms": _stats([p[0] + p[2] for p in hp]),
        "D_wall_ms": _stats(d), "D_cigar_ms": _stats([p[0] for p in parts]), "D_kernel_ms": _stats([p[1] for p in parts]),
        "D_download_ms": _stats([p[2] for p in parts]),
        "S_wall_ms": _stats(s), "S_cigar_ms": _stats([p[0] for p in sparts]), "S_kernel_ms": _stats([p[1] for p in sparts]),
        "S_download_ms": _stats([p[2] for p in sparts]),
        "S_sort_step_ms": round(statistics.median([p[1] for p in sparts]) - statistics.median([p[1] for p in parts]), 3),
        "record_bytes": nbytes, "nm_carry_out": host_carry,
        "sha256_H": sorted(digests["H"]), "sha256_D": sorted(digests["D"]), "sha256_S": sorted(digests["S"]),
        "sha256_H_sorted": want_sorted,
        "digests_equal": len(digests["H"]) == 1 and digests["H"] == digests["D"] and digests["S"] == {want_sorted},
    })
    print("RESULT " + json.dumps(out), flush=True)


def _cigars(snapgpu, base, r0, r1, loc, dr):
    cig = snapgpu.Cigars.empty(2 * r0.n)
    for e, r in enumerate((r0, r1)):
        k = base.Cigars(r, loc[e::2], dr[e::2])
        cig.editDistance[e::2], cig.nOps[e::2], cig.ops[e::2] = k.editDistance, k.nOps, k.ops
    return cig


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=C2["pairs"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "paired_bam.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be at least 3")
    if args.child:
        child(args.reps, args.pairs, args.genome_bases)
        return 0
    report = {"tool": "tools/paired_bam_time.py", "reps": args.reps, "pairs": args.pairs, "genome_bases": args.genome_bases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for threads in (16, 2):
        name = f"threads_{threads}"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--pairs", str(args.pairs),
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
    a, b = report["threads_16"], report["threads_2"]
    report["digests_equal"] = a["digests_equal"] and b["digests_equal"] and a["sha256_H"] == b["sha256_H"]
    for k, r in (("16", a), ("2", b)):
        report[f"D_wall_median_ms_{k}_threads"] = r["D_wall_ms"]["median"]
        report[f"S_wall_median_ms_{k}_threads"] = r["S_wall_ms"]["median"]
        report[f"H_wall_median_ms_{k}_threads"] = r["H_wall_ms"]["median"]
        report[f"H_format_median_ms_{k}_threads"] = r["H_format_ms"]["median"]
    save()
    print(f"16 threads: D {a['D_wall_ms']['median']} ms, S {a['S_wall_ms']['median']} ms, H {a['H_wall_ms']['median']} ms; "
          f"2 threads: D {b['D_wall_ms']['median']} ms, S {b['S_wall_ms']['median']} ms, H {b['H_wall_ms']['median']} ms; "
          f"digests equal: {report['digests_equal']}", flush=True)
    if not report["digests_equal"]:
        print("RECORDS DIFFER", flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
