#!/usr/bin/env python3
"""Time of the BAM records of 1M aligned reads: the host encoder against the device encoder, and
the BGZF compression that follows either.

bench.py's C2 workload (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99), ids r<i>.  Every
child process builds the world, aligns the reads and computes their CIGARs once on the GPU, then
times (the C calls only, each writing into a fresh uninitialised buffer), warm medians of `--reps`
after one warm-up of each leg:

  D    snapgpu_bam_resident + snapgpu_bam_download: wall time from the first call to the records in
       host memory, the kernel ms (all passes, HIP events) and the download ms;
  H16  snapgpu_bam_format on 16 host threads (SNAPGPU_HOST_THREADS=16), alternating with D;
  H2   the same on 2 host threads, a rank's share of the host on an 8-GPU node (the budget is read
       once per process, so it is a child of its own);
  Z16  snapgpu_bgzf_compress of the records (with the EOF block) on 16 host threads;
  Z1   the same on 1 host thread (a child of its own).

D's bytes must equal H's, and Z1's must equal Z16's (SHA-256).  There is no threshold: the report
states D against H16.  Medians and the spread go to --out, rewritten after every child.

Every child runs under its own time limit and the first one that fails, faults or times out ends
the run: nothing is started on a GPU after a failure.

    python3 tools/bam_format_time.py --reps 5 --out profiles/r11/bam_format.json
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
    res = dev.results()
    cig = dev.cigars()
    out = {"mode": mode, "host_threads": snapgpu.host_threads(), "reads": n}
    cap = int(lens.sum()) + 2 * int(reads._p.contents.totalBytes) + n * 512
    used, carry = C.c_uint64(), C.c_int32()

    def host(keep=False):
        buf = np.empty(cap, dtype=np.uint8)
        t = time.perf_counter()
        rc = lib.snapgpu_bam_format(idx._h, reads._p, blob, offs.ctypes.data, lens.ctypes.data, res.ctypes.data,
                                    cig.editDistance.ctypes.data, cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ",
                                    None, None, 0, C.byref(carry), buf.ctypes.data, cap, C.byref(used))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0, snapgpu.last_error()
        return ms, (buf[:used.value].copy() if keep else hashlib.sha256(buf[:used.value]).hexdigest()), used.value

    def device():
        t = time.perf_counter()
        rc = lib.snapgpu_bam_resident(al._h, dev._h, reads._p, blob, offs.ctypes.data, lens.ctypes.data, b"FASTQ", 0)
        assert rc == 0, snapgpu.last_error()
        lib.snapgpu_bam_download(al._h, dev._h, None, 0, C.byref(used), None)
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        rc = lib.snapgpu_bam_download(al._h, dev._h, buf.ctypes.data, used.value, C.byref(used), C.byref(carry))
        assert rc == 0, snapgpu.last_error()
        dev.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        k, d = al.bam_ms()
        return ms, hashlib.sha256(buf[:used.value]).hexdigest(), used.value, k, d

    def bgzf(records):
        zcap = len(records) + (len(records) // 0xff00 + 1) * 128 + 256
        zbuf = np.empty(zcap, dtype=np.uint8)
        t = time.perf_counter()
        rc = lib.snapgpu_bgzf_compress(records.ctypes.data, len(records), 1, zbuf.ctypes.data, zcap, C.byref(used))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0, snapgpu.last_error()
        return ms, hashlib.sha256(zbuf[:used.value]).hexdigest(), used.value

    if mode == "bgzf":
        _, records, nbytes = host(keep=True)
        bgzf(records)   # warm-up
        z, digests = [], set()
        for _ in range(reps):
            ms, h, zbytes = bgzf(records)
            z.append(ms)
            digests.add(h)
        out.update({"Z_ms": _stats(z), "record_bytes": nbytes, "bgzf_bytes": zbytes, "sha256_bgzf": sorted(digests),
                    "Z_input_MBps": round(nbytes / statistics.median(z) / 1e3, 1)})
        print("RESULT " + json.dumps(out), flush=True)
        return

    host()   # warm-up
    h_ms, digests = [], set()
    if mode == "ab":
        device()
        d_ms, kern, down = [], [], []
        for _ in range(reps):
            ms, h, nbytes = host()
            h_ms.append(ms)
            digests.add(h)
            ms, h, nb, k, d = device()
            assert nb == nbytes
            d_ms.append(ms)
            kern.append(k)
            down.append(d)
            digests.add(h)
        _, records, _ = host(keep=True)
        bgzf(records)   # warm-up
        z, zd = [], set()
        for _ in range(reps):
            ms, h, zbytes = bgzf(records)
            z.append(ms)
            zd.add(h)
        out.update({"D_wall_ms": _stats(d_ms), "D_kernel_ms": _stats(kern), "D_download_ms": _stats(down),
                    "Z_ms": _stats(z), "bgzf_bytes": zbytes, "sha256_bgzf": sorted(zd),
                    "Z_input_MBps": round(nbytes / statistics.median(z) / 1e3, 1)})
    else:
        for _ in range(reps):
            ms, h, nbytes = host()
            h_ms.append(ms)
            digests.add(h)
    out.update({"H_ms": _stats(h_ms), "record_bytes": nbytes, "sha256": sorted(digests), "digests_equal": len(digests) == 1,
                "H_records_per_s": round(n / statistics.median(h_ms) * 1e3)})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "bam_format.json"))
    ap.add_argument("--child", choices=("ab", "host", "bgzf"))
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be at least 3")
    if args.child:
        child(args.child, args.reps, args.reads, args.genome_bases)
        return 0

    report = {"tool": "tools/bam_format_time.py", "reps": args.reps, "reads": args.reads, "genome_bases": args.genome_bases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for name, mode, threads in (("D_and_H16_and_Z16", "ab", 16), ("H2", "host", 2), ("Z1", "bgzf", 1)):
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
    ab, h2, z1 = report["D_and_H16_and_Z16"], report["H2"], report["Z1"]
    report["digests_equal"] = (ab["digests_equal"] and h2["digests_equal"] and ab["sha256"] == h2["sha256"] and
                               len(z1["sha256_bgzf"]) == 1 and ab["sha256_bgzf"] == z1["sha256_bgzf"])
    report["D_wall_median_ms"] = ab["D_wall_ms"]["median"]
    report["H16_median_ms"] = ab["H_ms"]["median"]
    report["H2_median_ms"] = h2["H_ms"]["median"]
    report["Z16_median_ms"] = ab["Z_ms"]["median"]
    report["Z1_median_ms"] = z1["Z_ms"]["median"]
    report["D_median_above_H16_median"] = ab["D_wall_ms"]["median"] > ab["H_ms"]["median"]
    save()
    print(f"D wall {report['D_wall_median_ms']} ms, H16 {report['H16_median_ms']} ms, H2 {report['H2_median_ms']} ms, "
          f"Z16 {report['Z16_median_ms']} ms, Z1 {report['Z1_median_ms']} ms; digests equal: {report['digests_equal']}", flush=True)
    if not report["digests_equal"]:
        print("BYTES DIFFER", flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
