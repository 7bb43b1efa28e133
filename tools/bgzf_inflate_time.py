#!/usr/bin/env python3
"""Time from a BGZF-compressed FASTQ file to a resident read batch: zlib on the host threads + the
device parser against the device inflater + the device parser.

bench.py's C2 reads (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99) written with write_fastq
and compressed as bgzip does: members of 0xff00 bytes, zlib level 6 (both files stay in the page cache
for every leg).  The aligner only owns the streams and buffers here, so it is built over a 1 Mb index.
Every child process writes the files, then times, after `--warmup` untimed runs, `--reps` runs of its leg:

  H16  snapgpu_bgzf_inflate of the compressed file's bytes on 16 host threads (SNAPGPU_HOST_THREADS=16), then
       snapgpu_fastq_upload of the text without host batch: inflate ms, upload ms and their sum;
  H2   the same on 2 host threads, a rank's share of the host on an 8-GPU node;
  D16  BaseAligner.upload_fastq(path, bgzf=True) without and with the host batch, 16 host threads for the
       host passes (file -> memory -> pinned staging): wall ms, snapgpu_fastq_last_ms' split into upload,
       kernels and downloads, and the inflate kernel's own ms (snapgpu_bgzf_inflate_last_ms);
  D2   the same on 2 host threads;
  P16  for scale: BaseAligner.upload_fastq(path) of the plain text, without and with the host batch.

All legs' batches must be equal (the resident extent hash; SHA-256 over every field of the host batch where
there is one).  Medians and the spread go to --out, rewritten after every child.  Every child runs under
its own time limit and the first one that fails, faults or times out ends the run: nothing is started on a
GPU after a failure.

    python3 tools/bgzf_inflate_time.py --out profiles/r16/bgzf_inflate.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fastq_parse_time import C2, _digest, _stats  # noqa: E402

CHILD_LIMIT_S = 300
BLOCK = 0xff00


def bgzip(text, level=6):
    """`text` as bgzip writes it: members of 0xff00 bytes at zlib level 6, then the EOF block."""
    from inflate_cases import member

    def one(k):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        piece = text[k:k + BLOCK]
        return member(c.compress(piece) + c.flush(), piece)
    with ThreadPoolExecutor(16) as pool:
        parts = list(pool.map(one, range(0, len(text), BLOCK)))
    return b"".join(parts) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def child(mode, reps, warmup, n_reads, genome_bases, clipping):
    import numpy as np
    import snapgpu
    from fastq_cases import batch_fields
    g = snapgpu.Genome.synthetic(genome_bases, seed=2121, n_contigs=C2["n_contigs"], n_repeat_families=C2["families"])
    small = snapgpu.Genome.synthetic(1_000_000, seed=2121, n_contigs=3, n_repeat_families=60)
    al = snapgpu.BaseAligner(snapgpu.GenomeIndex.build(small, 20, 8))
    lib = snapgpu.lib()
    with tempfile.TemporaryDirectory() as tmp:
        path, gz = os.path.join(tmp, "c2.fq"), os.path.join(tmp, "c2.fq.gz")
        snapgpu.Reads.synthetic(g, n_reads, seed=99).write_fastq(path)
        text = open(path, "rb").read()
        stream = bgzip(text)
        open(gz, "wb").write(stream)
        size, members = snapgpu.bgzf_inflate_size(stream)
        assert size == len(text)
        out = {"mode": mode, "host_threads": snapgpu.host_threads(), "reads": n_reads, "clipping": clipping,
               "text_bytes": len(text), "compressed_bytes": len(stream), "members": members,
               "ratio": round(len(stream) / len(text), 4), "inflate_waves": al.bgzf_inflate_waves()}
        del text

        def host():
            src = np.fromfile(gz, dtype=np.uint8)          # the file from the page cache, as the device legs read it
            buf = np.empty(size, dtype=np.uint8)
            used, d = C.c_uint64(), C.c_void_p()
            t0 = time.perf_counter()
            assert lib.snapgpu_bgzf_inflate(src.ctypes.data, src.size, buf.ctypes.data, size, C.byref(used)) == 0
            t1 = time.perf_counter()
            assert lib.snapgpu_fastq_upload(al._h, buf.ctypes.data, used.value, b"c2", clipping, 0, C.byref(d), None) == 0
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, snapgpu.DeviceReads(al, None, handle=d.value)

        def device(source, host_batch, bgzf):
            t0 = time.perf_counter()
            dev = al.upload_fastq(source, clipping=clipping, host_batch=host_batch, bgzf=bgzf)
            ms = (time.perf_counter() - t0) * 1e3
            return ms, al.fastq_last_ms() + ((al.bgzf_inflate_ms()[1],) if bgzf else (0.0,)), dev

        if mode == "host":
            for _ in range(warmup):
                host()
            inflate, up = [], []
            for _ in range(reps):
                i, u, dev = host()
                inflate.append(i)
                up.append(u)
            out.update({"inflate_ms": _stats(inflate), "upload_fastq_ms": _stats(up),
                        "sum_ms": _stats([i + u for i, u in zip(inflate, up)]),
                        "extent_hash": dev.peek(arrays=False)["extentHash"]})
        else:
            source, bgzf = (gz, True) if mode == "device" else (path, False)
            for _ in range(warmup):
                device(source, False, bgzf)
                device(source, True, bgzf)
            for key, hb in (("without_host_batch", False), ("with_host_batch", True)):
                wall, split = [], []
                for _ in range(reps):
                    ms, parts, dev = device(source, hb, bgzf)
                    wall.append(ms)
                    split.append(parts)
                out[key] = {"wall_ms": _stats(wall), "upload_ms": _stats([s[0] for s in split]),
                            "kernel_ms": _stats([s[1] for s in split]), "download_ms": _stats([s[2] for s in split]),
                            "extent_hash": dev.peek(arrays=False)["extentHash"]}
                if bgzf:
                    out[key]["inflate_kernel_ms"] = _stats([s[3] for s in split])
                if hb:
                    out[key]["sha256"] = _digest(batch_fields(dev.reads))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--clipping", type=int, default=3, help="ReadClippingType applied by every leg (the reference default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "bgzf_inflate.json"))
    ap.add_argument("--child", choices=("host", "device", "plain"))
    args = ap.parse_args()
    if args.reps < 5 or args.warmup < 1:
        ap.error("--reps must be at least 5 and --warmup at least 1")
    if args.child:
        child(args.child, args.reps, args.warmup, args.reads, args.genome_bases, args.clipping)
        return 0

    report = {"tool": "tools/bgzf_inflate_time.py", "reps": args.reps, "warmup": args.warmup, "reads": args.reads,
              "genome_bases": args.genome_bases, "clipping": args.clipping, "block_bytes": BLOCK, "zlib_level": 6}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    legs = (("H16", "host", 16), ("H2", "host", 2), ("D16", "device", 16), ("D2", "device", 2), ("P16", "plain", 16))
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
    batched = [report[k][hb] for k in ("D16", "D2", "P16") for hb in ("without_host_batch", "with_host_batch")]
    hashes = {report["H16"]["extent_hash"], report["H2"]["extent_hash"]} | {b["extent_hash"] for b in batched}
    digests = {b["sha256"] for b in batched if "sha256" in b}
    report["batches_equal"] = len(hashes) == 1 and len(digests) == 1
    for k in ("H16", "H2"):
        report[f"{k}_inflate_plus_upload_median_ms"] = report[k]["sum_ms"]["median"]
    for k in ("D16", "D2", "P16"):
        for hb in ("without_host_batch", "with_host_batch"):
            report[f"{k}_{hb}_median_ms"] = report[k][hb]["wall_ms"]["median"]
    save()
    print(json.dumps({k: v for k, v in report.items() if k.endswith("_ms") or k == "batches_equal"}), flush=True)
    if not report["batches_equal"]:
        print("BATCHES DIFFER", flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
