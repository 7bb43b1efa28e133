#!/usr/bin/env python3
"""Time from a FASTQ file to SAM text and to a BGZF-compressed BAM stream in host memory, with and
without a host read batch between the device parser and the device formatters.

bench.py's C2 workload (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99): the reads written with
write_fastq, as plain text and compressed as bgzip does (both files stay in the page cache).  Every
child process builds the world, then times, after `--warmup` untimed runs, `--reps` runs of its leg on
each of the two files.  A run goes from the file to (i) the SAM text in host memory (parse / upload, run,
run_cigars, run_sam, sam) and, separately, from the file to (ii) the BGZF stream in host memory (parse /
upload, run, run_cigars, run_bam, run_bgzf, bgzf):

  H16  the host parser (snapgpu_bgzf_inflate first for the compressed file) + clip + BaseAligner.upload,
       the formatters with the host batch, on 16 host threads (SNAPGPU_HOST_THREADS=16);
  H2   the same on 2 host threads, a rank's share of the host on an 8-GPU node;
  B16  BaseAligner.upload_fastq(path, host_batch=True), the formatters with the batch it downloaded;
  B2   the same on 2 host threads;
  D16  BaseAligner.upload_fastq(path, host_batch=False), the formatters with reads=None: the ids, clip
       arrays and the unclipped tail stay in device memory;
  D2   the same on 2 host threads.

All legs' SAM texts and all legs' BGZF streams must be equal (SHA-256).  Medians and the spread go to
--out, rewritten after every child.  Every child runs under its own time limit and the first one that
fails, faults or times out ends the run: nothing is started on a GPU after a failure.

    python3 tools/fastq_to_bam_time.py --out profiles/r18/fastq_to_bam.json
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bgzf_inflate_time import bgzip  # noqa: E402
from fastq_parse_time import C2, _stats  # noqa: E402

CHILD_LIMIT_S = 420


def child(mode, reps, warmup, n_reads, genome_bases, clipping):
    import snapgpu
    g = snapgpu.Genome.synthetic(genome_bases, seed=2121, n_contigs=C2["n_contigs"], n_repeat_families=C2["families"])
    idx = snapgpu.GenomeIndex.build(g, 20, 16, device=0)
    al = snapgpu.BaseAligner(idx)
    with tempfile.TemporaryDirectory() as tmp:
        path, gz = os.path.join(tmp, "c2.fq"), os.path.join(tmp, "c2.fq.gz")
        snapgpu.Reads.synthetic(idx.genome_handle(), n_reads, seed=99).write_fastq(path)
        text = open(path, "rb").read()
        open(gz, "wb").write(bgzip(text))
        out = {"mode": mode, "host_threads": snapgpu.host_threads(), "reads": n_reads, "clipping": clipping,
               "text_bytes": len(text), "compressed_bytes": os.path.getsize(gz)}
        del text

        def arrive(source, bgzf):
            """-> (the resident batch, what the formatters take as `reads`)"""
            if mode == "host":
                data = open(source, "rb").read()
                reads = snapgpu.Reads.from_fastq_bytes(snapgpu.bgzf_inflate(data), name=source) if bgzf else \
                    snapgpu.Reads.from_fastq(source)
                if clipping:
                    reads.clip(clipping)
                return al.upload(reads), reads
            dev = al.upload_fastq(source, clipping=clipping, host_batch=mode == "batch", bgzf=bgzf)
            return dev, dev.reads

        def run(source, bgzf, want):
            t0 = time.perf_counter()
            dev, reads = arrive(source, bgzf)
            t1 = time.perf_counter()
            dev.run()
            dev.run_cigars()
            done = {}
            if want == "sam":
                dev.run_sam(reads)
                data = dev.sam(timing=done)
            else:
                dev.run_bam(reads)
                dev.run_bgzf()
                data = dev.bgzf(timing=done)
            ms = (done["done"] - t0) * 1e3
            dev.synchronize()
            return ms, (t1 - t0) * 1e3, hashlib.sha256(data).hexdigest(), len(data)

        for name, source, bgzf in (("plain", path, False), ("bgzf", gz, True)):
            for _ in range(warmup):
                run(source, bgzf, "sam")
                run(source, bgzf, "bgzf")
            leg = {}
            for want in ("sam", "bgzf"):
                wall, arrival, digests = [], [], set()
                for _ in range(reps):
                    ms, up, h, nbytes = run(source, bgzf, want)
                    wall.append(ms)
                    arrival.append(up)
                    digests.add(h)
                leg["to_" + want] = {"wall_ms": _stats(wall), "arrival_ms": _stats(arrival), "bytes": nbytes,
                                     "sha256": sorted(digests)}
            out[name] = leg
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--clipping", type=int, default=3, help="ReadClippingType applied by every leg (the reference default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "fastq_to_bam.json"))
    ap.add_argument("--child", choices=("host", "batch", "device"))
    args = ap.parse_args()
    if args.reps < 5 or args.warmup < 1:
        ap.error("--reps must be at least 5 and --warmup at least 1")
    if args.child:
        child(args.child, args.reps, args.warmup, args.reads, args.genome_bases, args.clipping)
        return 0

    report = {"tool": "tools/fastq_to_bam_time.py", "reps": args.reps, "warmup": args.warmup, "reads": args.reads,
              "genome_bases": args.genome_bases, "clipping": args.clipping}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    legs = (("H16", "host", 16), ("H2", "host", 2), ("B16", "batch", 16), ("B2", "batch", 2), ("D16", "device", 16),
            ("D2", "device", 2))
    for name, mode, threads in legs:
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
    names = [leg[0] for leg in legs]
    equal = True
    for want in ("to_sam", "to_bgzf"):
        digests = {h for k in names for src in ("plain", "bgzf") for h in report[k][src][want]["sha256"]}
        equal = equal and len(digests) == 1
    report["outputs_equal"] = equal
    for k in names:
        for src in ("plain", "bgzf"):
            for want in ("to_sam", "to_bgzf"):
                report[f"{k}_{src}_{want}_median_ms"] = report[k][src][want]["wall_ms"]["median"]
    for t in ("16", "2"):
        for src in ("plain", "bgzf"):
            for want in ("to_sam", "to_bgzf"):
                report[f"D{t}_saves_over_B{t}_{src}_{want}_ms"] = round(
                    report[f"B{t}_{src}_{want}_median_ms"] - report[f"D{t}_{src}_{want}_median_ms"], 3)
    save()
    print(json.dumps({k: v for k, v in report.items() if k.endswith("_ms") or k == "outputs_equal"}), flush=True)
    if not equal:
        print("OUTPUTS DIFFER", flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
