#!/usr/bin/env python3
"""Time from a FASTQ file to a resident read batch: the host parser + upload against the device parser.

bench.py's C2 reads (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99) written with write_fastq
(the file stays in the page cache for every leg).  The aligner only owns the streams and buffers here,
so it is built over a 1 Mb index.  Every child process writes the file, then times, after `--warmup`
untimed runs, `--reps` runs of its leg:

  A16  Reads.from_fastq + BaseAligner.upload on 16 host threads (SNAPGPU_HOST_THREADS=16): parse ms,
       upload ms and their sum;
  A2   the same on 2 host threads, a rank's share of the host on an 8-GPU node (the budget is read once
       per process, so it is a child of its own);
  B16  BaseAligner.upload_fastq(path) with and without the host batch, 16 host threads for the one host
       pass (file -> pinned staging): wall ms and snapgpu_fastq_last_ms' split into text upload,
       kernels (HIP events; also by pass) and downloads;
  B2   the same on 2 host threads.

B's batch must equal A's (SHA-256 over every field of the host batch, and the resident extent hash).
Medians and the spread go to --out, rewritten after every child.  Every child runs under its own time
limit and the first one that fails, faults or times out ends the run: nothing is started on a GPU after
a failure.

    python3 tools/fastq_parse_time.py --reps 5 --out profiles/r14/fastq_parse.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

# bench.py WORKLOADS["c2"]
C2 = dict(genome_bases=46_709_983, n_contigs=1, families=200, reads=1_000_000)
CHILD_LIMIT_S = 300
PASSES = ("newline_count", "tile_scan", "line_starts", "records", "length_scans", "copy")


def _stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]}


def _digest(fields):
    h = hashlib.sha256()
    for k in sorted(fields):
        v = fields[k]
        h.update(k.encode() + b"=" + (b"NULL" if v is None else v.tobytes() if hasattr(v, "tobytes") else
                                     v if isinstance(v, bytes) else str(v).encode()) + b";")
    return h.hexdigest()


def child(mode, reps, warmup, n_reads, genome_bases, clipping):
    import snapgpu
    from fastq_cases import batch_fields
    g = snapgpu.Genome.synthetic(genome_bases, seed=2121, n_contigs=C2["n_contigs"], n_repeat_families=C2["families"])
    small = snapgpu.Genome.synthetic(1_000_000, seed=2121, n_contigs=3, n_repeat_families=60)
    al = snapgpu.BaseAligner(snapgpu.GenomeIndex.build(small, 20, 8))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "c2.fq")
        snapgpu.Reads.synthetic(g, n_reads, seed=99).write_fastq(path)
        out = {"mode": mode, "host_threads": snapgpu.host_threads(), "reads": n_reads, "clipping": clipping,
               "file_bytes": os.path.getsize(path)}

        pass_ms = snapgpu.lib().snapgpu_internal_fastq_pass_ms
        pass_ms.restype, pass_ms.argtypes = C.c_int, [C.c_void_p, C.c_void_p]

        def host():
            t0 = time.perf_counter()
            reads = snapgpu.Reads.from_fastq(path)
            if clipping:
                reads.clip(clipping)
            t1 = time.perf_counter()
            dev = al.upload(reads)
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, reads, dev

        def device(host_batch):
            t0 = time.perf_counter()
            dev = al.upload_fastq(path, clipping=clipping, host_batch=host_batch)
            ms = (time.perf_counter() - t0) * 1e3
            passes = (C.c_double * 6)()
            assert pass_ms(al._h, passes) == 0
            return ms, al.fastq_last_ms() + (list(passes),), dev

        if mode == "host":
            for _ in range(warmup):
                host()
            parse, up = [], []
            for _ in range(reps):
                p, u, reads, dev = host()
                parse.append(p)
                up.append(u)
            out.update({"parse_ms": _stats(parse), "upload_ms": _stats(up), "sum_ms": _stats([p + u for p, u in zip(parse, up)]),
                        "sha256": _digest(batch_fields(reads)), "extent_hash": dev.peek(arrays=False)["extentHash"]})
        else:
            for _ in range(warmup):
                device(True)
                device(False)
            for key, hb in (("with_host_batch", True), ("without_host_batch", False)):
                wall, split = [], []
                for _ in range(reps):
                    ms, parts, dev = device(hb)
                    wall.append(ms)
                    split.append(parts)
                out[key] = {"wall_ms": _stats(wall), "text_upload_ms": _stats([s[0] for s in split]),
                            "kernel_ms": _stats([s[1] for s in split]), "download_ms": _stats([s[2] for s in split]),
                            "pass_ms": {name: _stats([s[3][i] for s in split]) for i, name in enumerate(PASSES)},
                            "extent_hash": dev.peek(arrays=False)["extentHash"]}
                if hb:
                    out[key]["sha256"] = _digest(batch_fields(dev.reads))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--clipping", type=int, default=3, help="ReadClippingType applied by both paths (the reference default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "fastq_parse.json"))
    ap.add_argument("--child", choices=("host", "device"))
    args = ap.parse_args()
    if args.reps < 5 or args.warmup < 1:
        ap.error("--reps must be at least 5 and --warmup at least 1")
    if args.child:
        child(args.child, args.reps, args.warmup, args.reads, args.genome_bases, args.clipping)
        return 0

    report = {"tool": "tools/fastq_parse_time.py", "reps": args.reps, "warmup": args.warmup, "reads": args.reads,
              "genome_bases": args.genome_bases, "clipping": args.clipping}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for name, mode, threads in (("A16", "host", 16), ("A2", "host", 2), ("B16", "device", 16), ("B2", "device", 2)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(args.reps), "--warmup",
               str(args.warmup), "--reads", str(args.reads), "--genome-bases", str(args.genome_bases), "--clipping",
               str(args.clipping)]
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
    a16, a2, b16, b2 = (report[k] for k in ("A16", "A2", "B16", "B2"))
    digests = {a16["sha256"], a2["sha256"], b16["with_host_batch"]["sha256"], b2["with_host_batch"]["sha256"]}
    hashes = {a16["extent_hash"], a2["extent_hash"]} | {b[k]["extent_hash"] for b in (b16, b2)
                                                        for k in ("with_host_batch", "without_host_batch")}
    report["batches_equal"] = len(digests) == 1 and len(hashes) == 1
    for k, r in (("A16", a16), ("A2", a2)):
        report[f"{k}_parse_plus_upload_median_ms"] = r["sum_ms"]["median"]
    for k, r in (("B16", b16), ("B2", b2)):
        report[f"{k}_with_host_batch_median_ms"] = r["with_host_batch"]["wall_ms"]["median"]
        report[f"{k}_without_host_batch_median_ms"] = r["without_host_batch"]["wall_ms"]["median"]
    save()
    print(json.dumps({k: v for k, v in report.items() if k.endswith("_ms") or k == "batches_equal"}), flush=True)
    if not report["batches_equal"]:
        print("BATCHES DIFFER", flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
