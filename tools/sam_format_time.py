#!/usr/bin/env python3
"""Time of the SAM text of 1M aligned reads: the host formatter against the device formatter.

bench.py's C2 workload (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99), ids r<i>.  Every
child process builds the world, aligns the reads and computes their CIGARs once on the GPU, then
times (the C calls only, each writing into a fresh uninitialised buffer):

  A16  snapgpu_sam_format on 16 host threads (SNAPGPU_HOST_THREADS=16);
  A2   the same on 2 host threads, a rank's share of the host on an 8-GPU node (the budget is read
       once per process, so it is a child of its own);
  B    snapgpu_sam_resident + snapgpu_sam_download: wall time from the first call to the text in
       host memory, the kernel ms (length + scan + write, HIP events; also by pass) and the download ms.

The "ab" child alternates A16 and B `--reps` times after one warm-up of each; it also records the
D2H of the records and CIGAR rows that A needs and B does not, and snapgpu_copy_peak.  B's bytes
must equal A's (SHA-256).  Medians and the spread go to --out, rewritten after every child.

--sorted measures coordinate-sorted output (`-so`) instead, in one child that alternates two legs
`--reps` times after one warm-up of each:

  S      snapgpu_sam_resident_sorted + snapgpu_sam_download: wall time, kernel ms by pass and the
         sort step's ms (snapgpu_sam_sort_ms);
  B + H  the unsorted device path B as above, then snapgpu_sam_sort_records on its text (H, one host
         thread by construction).

S's bytes must equal B + H's (SHA-256).  No threshold: the report states S against B + H.

Every child runs under its own time limit and the first one that fails, faults or times out ends
the run: nothing is started on a GPU after a failure.

    python3 tools/sam_format_time.py --reps 5 --out profiles/r07/sam_format.json
    python3 tools/sam_format_time.py --reps 5 --sorted --out profiles/r10/sam_sorted.json
"""
import argparse
import ctypes as C
import hashlib
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


def _stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def child(mode, reps, n_reads, genome_bases):
    import numpy as np
    import snapgpu
    lib = snapgpu.lib()
    g = snapgpu.Genome.synthetic(genome_bases, seed=2121, n_contigs=C2["n_contigs"], n_repeat_families=C2["families"])
    idx = snapgpu.GenomeIndex.build(g, 20, 16, device=0)
    reads = snapgpu.Reads.synthetic(idx.genome_handle(), n_reads, seed=99)
    n = reads.n
    blob, offs, lens = snapgpu._id_arrays([b"r%d" % i for i in range(n)], n)
    al = snapgpu.BaseAligner(idx)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    dev.synchronize()
    t0 = time.perf_counter()
    res = dev.results()
    cig = dev.cigars()
    d2h_ms = (time.perf_counter() - t0) * 1e3
    out = {"mode": mode, "host_threads": snapgpu.host_threads(), "reads": n,
           "records_and_cigar_rows_d2h_ms": round(d2h_ms, 3), "records_and_cigar_rows_bytes": n * (64 + 4 + 4 + 256)}
    cap = int(lens.sum()) + 2 * int(reads._p.contents.totalBytes) + n * 512
    used = C.c_uint64()

    def host():
        buf = np.empty(cap, dtype=np.uint8)
        t = time.perf_counter()
        rc = lib.snapgpu_sam_format(idx._h, reads._p, blob, offs.ctypes.data, lens.ctypes.data, res.ctypes.data,
                                    cig.editDistance.ctypes.data, cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ",
                                    buf.ctypes.data, cap, C.byref(used))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0, snapgpu.last_error()
        return ms, hashlib.sha256(buf[:used.value]).hexdigest(), used.value

    def device(sorted_output=False, keep=False):
        fn = lib.snapgpu_sam_resident_sorted if sorted_output else lib.snapgpu_sam_resident
        t = time.perf_counter()
        rc = fn(al._h, dev._h, reads._p, blob, offs.ctypes.data, lens.ctypes.data, b"FASTQ")
        assert rc == 0, snapgpu.last_error()
        lib.snapgpu_sam_download(al._h, dev._h, None, 0, C.byref(used))
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        rc = lib.snapgpu_sam_download(al._h, dev._h, buf.ctypes.data, used.value, C.byref(used))
        assert rc == 0, snapgpu.last_error()
        dev.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        k, d = al.sam_ms()
        if keep:   # the text itself, for the host sorter
            return ms, buf[:used.value], k, d, al.sam_pass_ms()
        return ms, hashlib.sha256(buf[:used.value]).hexdigest(), used.value, k, d, al.sam_pass_ms()

    def host_sort(text):
        out_buf = np.empty(max(1, len(text)), dtype=np.uint8)
        t = time.perf_counter()
        rc = lib.snapgpu_sam_sort_records(idx._h, text.ctypes.data_as(C.c_char_p), len(text),
                                          out_buf.ctypes.data_as(C.c_char_p), len(text), C.byref(used))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0 and used.value == len(text), snapgpu.last_error()
        return ms, hashlib.sha256(out_buf[:len(text)]).hexdigest()

    if mode == "sorted":
        device(True)
        host_sort(device(keep=True)[1])   # warm-up of both legs
        S, B, H, sort_ms, kern = [], [], [], [], {"S": [], "B": []}
        passes = {"S": [], "B": []}
        digests = {"S": set(), "BH": set()}
        for _ in range(reps):
            ms, h, nbytes, k, d, ps = device(True)
            S.append(ms)
            sort_ms.append(al.sam_sort_ms())
            kern["S"].append(k)
            passes["S"].append(ps)
            digests["S"].add(h)
            ms, text, k, d, ps = device(keep=True)
            assert len(text) == nbytes
            B.append(ms)
            kern["B"].append(k)
            passes["B"].append(ps)
            ms, h = host_sort(text)
            H.append(ms)
            digests["BH"].add(h)
        bh = [b + h for b, h in zip(B, H)]
        pass_stats = lambda v: {name: _stats([p[i] for p in v]) for i, name in enumerate(("length", "scan", "write"))}
        out.update({
            "S_wall_ms": _stats(S), "B_wall_ms": _stats(B), "H_host_sort_ms": _stats(H), "B_plus_H_ms": _stats(bh),
            "S_sort_ms": _stats(sort_ms), "S_kernel_ms": _stats(kern["S"]), "B_kernel_ms": _stats(kern["B"]),
            "S_pass_ms": pass_stats(passes["S"]), "B_pass_ms": pass_stats(passes["B"]),
            "sorted_write_over_unsorted_write": round(statistics.median(p[2] for p in passes["S"]) /
                                                      statistics.median(p[2] for p in passes["B"]), 3),
            "text_bytes": nbytes, "sha256_S": sorted(digests["S"]), "sha256_B_plus_H": sorted(digests["BH"]),
            "digests_equal": len(digests["S"]) == 1 and digests["S"] == digests["BH"],
            "S_median_above_B_plus_H_median": statistics.median(S) > statistics.median(bh),
        })
        print("RESULT " + json.dumps(out), flush=True)
        return

    host()   # warm-up
    a, b, digests = [], [], set()
    if mode == "ab":
        device()
        kern, down, passes = [], [], []
        for _ in range(reps):
            ms, h, nbytes = host()
            a.append(ms)
            digests.add(h)
            ms, h, nb, k, d, ps = device()
            assert nb == nbytes
            b.append(ms)
            kern.append(k)
            down.append(d)
            passes.append(ps)
            digests.add(h)
        peak_bytes = nbytes // 4096 * 4096
        peak_ms = al.copy_peak_ms(peak_bytes)
        write_ms = statistics.median(p[2] for p in passes)
        out.update({
            "B_wall_ms": _stats(b), "B_kernel_ms": _stats(kern), "B_download_ms": _stats(down),
            "B_pass_ms": {name: _stats([p[i] for p in passes]) for i, name in enumerate(("length", "scan", "write"))},
            "copy_peak": {"bytes_each_way": peak_bytes, "ms": round(peak_ms, 4),
                          "GBps_read_plus_write": round(2 * peak_bytes / peak_ms / 1e6, 1)},
            # the write pass reads ~ the text's bytes (ids, bases, qualities) and writes the text
            "write_pass_text_GBps": round(nbytes / write_ms / 1e6, 1),
            "write_pass_fraction_of_copy_peak": round((nbytes / write_ms) / (peak_bytes / peak_ms), 4),
        })
    else:
        for _ in range(reps):
            ms, h, nbytes = host()
            a.append(ms)
            digests.add(h)
    out.update({"A_ms": _stats(a), "text_bytes": nbytes, "sha256": sorted(digests), "digests_equal": len(digests) == 1,
                "A_lines_per_s": round(n / statistics.median(a) * 1e3)})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--out", help="default profiles/r07/sam_format.json, or profiles/r10/sam_sorted.json with --sorted")
    ap.add_argument("--sorted", action="store_true", help="coordinate-sorted output: S against B + H (see above)")
    ap.add_argument("--child", choices=("ab", "host", "sorted"))
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be at least 3")
    if args.child:
        child(args.child, args.reps, args.reads, args.genome_bases)
        return 0

    if not args.out:
        args.out = os.path.join(ROOT, "profiles", *(("r10", "sam_sorted.json") if args.sorted else ("r07", "sam_format.json")))
    report = {"tool": "tools/sam_format_time.py" + (" --sorted" if args.sorted else ""), "reps": args.reps, "reads": args.reads, "genome_bases": args.genome_bases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    legs = (("S_and_B_plus_H", "sorted", 16),) if args.sorted else (("A16_and_B", "ab", 16), ("A2", "host", 2))
    for name, mode, threads in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(args.reps), "--reads",
               str(args.reads), "--genome-bases", str(args.genome_bases)]
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
    if args.sorted:
        r = report["S_and_B_plus_H"]
        report["digests_equal"] = r["digests_equal"]
        report["S_wall_median_ms"] = r["S_wall_ms"]["median"]
        report["B_plus_H_median_ms"] = r["B_plus_H_ms"]["median"]
        save()
        print(f"S {r['S_wall_ms']['median']} ms (sort step {r['S_sort_ms']['median']} ms), B {r['B_wall_ms']['median']} ms + "
              f"H {r['H_host_sort_ms']['median']} ms; digests equal: {r['digests_equal']}", flush=True)
        if not r["digests_equal"]:
            print("TEXT DIFFERS", flush=True)
            return 2
        return 0
    ab, a2 = report["A16_and_B"], report["A2"]
    report["digests_equal"] = ab["digests_equal"] and a2["digests_equal"] and ab["sha256"] == a2["sha256"]
    report["A16_median_ms"] = ab["A_ms"]["median"]
    report["A2_median_ms"] = a2["A_ms"]["median"]
    report["B_wall_median_ms"] = ab["B_wall_ms"]["median"]
    report["B_wall_max_ms"] = ab["B_wall_ms"]["max"]
    # acceptance: B's wall time against A16's median of the same run -- by B's median, and rep by rep
    report["B_median_not_above_A16_median"] = ab["B_wall_ms"]["median"] <= ab["A_ms"]["median"]
    report["B_reps_above_A16_median"] = sum(1 for x in ab["B_wall_ms"]["all"] if x > ab["A_ms"]["median"])
    save()
    print(f"A16 {report['A16_median_ms']} ms, A2 {report['A2_median_ms']} ms, B wall {report['B_wall_median_ms']} ms "
          f"(max {report['B_wall_max_ms']}); digests equal: {report['digests_equal']}", flush=True)
    if not report["digests_equal"]:
        print("TEXT DIFFERS", flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
