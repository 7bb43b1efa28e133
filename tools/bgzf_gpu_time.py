#!/usr/bin/env python3
"""Time and size of the BGZF stream of 1M aligned reads' BAM records: compressed on the device from
the resident records against downloaded and compressed by zlib on the host threads.

bench.py's C2 workload (chr21-sized synthetic genome, 1M x 100 bp reads, seed 99), ids r<i>.  Every
child process builds the world, aligns the reads and computes their CIGARs once on the GPU, then
times (the C calls only), warm medians of `--reps` after one warm-up of each leg:

  G    snapgpu_bam_resident + snapgpu_bam_bgzf_resident + snapgpu_bam_bgzf_download: wall time from
       the first call to the compressed stream in host memory, the compressor's kernel ms (all passes
       and each pass, HIP events) and its download ms;
  P16  the path before the device compressor: snapgpu_bam_resident + snapgpu_bam_download of the
       records + snapgpu_bgzf_compress on 16 host threads (SNAPGPU_HOST_THREADS=16), alternating with G;
  P2   the same on 2 host threads, a rank's share of the host on an 8-GPU node (the budget is read
       once per process, so it is a child of its own).

The first child also records the sizes of the device stream, of the host's zlib level 6 stream and
of zlib level 1 over the same blocks, that every member of the device stream inflates to its slice
of the records, and that the stream equals the host model's.  There is no threshold: the report
states what was measured.  It goes to --out, rewritten after every child.

Every child runs under its own time limit and the first one that fails, faults or times out ends
the run: nothing is started on a GPU after a failure.

    python3 tools/bgzf_gpu_time.py --reps 5 --out profiles/r12/bgzf_gpu.json
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
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))

# bench.py WORKLOADS["c2"]
C2 = dict(genome_bases=46_709_983, n_contigs=1, families=200, reads=1_000_000)
CHILD_LIMIT_S = 420
BLOCK = 0xff00


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
    out = {"mode": mode, "host_threads": snapgpu.host_threads(), "reads": n}
    used = C.c_uint64()
    pass_ms = lib.snapgpu_internal_bgzf_pass_ms
    pass_ms.restype, pass_ms.argtypes = C.c_int, [C.c_void_p, C.c_void_p]

    def records_resident():
        rc = lib.snapgpu_bam_resident(al._h, dev._h, reads._p, blob, offs.ctypes.data, lens.ctypes.data, b"FASTQ", 0)
        assert rc == 0, snapgpu.last_error()

    def device(keep=False):
        t = time.perf_counter()
        records_resident()
        rc = lib.snapgpu_bam_bgzf_resident(al._h, dev._h)
        assert rc == 0, snapgpu.last_error()
        lib.snapgpu_bam_bgzf_download(al._h, dev._h, 1, None, 0, C.byref(used))
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        rc = lib.snapgpu_bam_bgzf_download(al._h, dev._h, 1, buf.ctypes.data, used.value, C.byref(used))
        assert rc == 0, snapgpu.last_error()
        ms = (time.perf_counter() - t) * 1e3
        k, d = al.bgzf_ms()
        passes = (C.c_double * 3)()
        assert pass_ms(al._h, passes) == 0
        stream = buf[:used.value]
        return ms, (stream.tobytes() if keep else hashlib.sha256(stream).hexdigest()), used.value, k, d, list(passes)

    def parent(keep=False):
        t = time.perf_counter()
        records_resident()
        lib.snapgpu_bam_download(al._h, dev._h, None, 0, C.byref(used), None)
        rec = np.empty(max(1, used.value), dtype=np.uint8)
        rc = lib.snapgpu_bam_download(al._h, dev._h, rec.ctypes.data, used.value, C.byref(used), None)
        assert rc == 0, snapgpu.last_error()
        nrec = used.value
        t1 = time.perf_counter()
        zcap = nrec + (nrec // BLOCK + 1) * 128 + 256
        zbuf = np.empty(zcap, dtype=np.uint8)
        rc = lib.snapgpu_bgzf_compress(rec.ctypes.data, nrec, 1, zbuf.ctypes.data, zcap, C.byref(used))
        assert rc == 0, snapgpu.last_error()
        t2 = time.perf_counter()
        return (t2 - t) * 1e3, (t2 - t1) * 1e3, (rec[:nrec].tobytes() if keep else None), nrec, used.value

    parent()   # warm-up
    p_ms, z_ms = [], []
    if mode == "ab":
        device()
        g_ms, kern, down, passes, digests = [], [], [], [], set()
        for _ in range(reps):
            ms, z, _, nrec, zbytes = parent()
            p_ms.append(ms)
            z_ms.append(z)
            ms, h, gbytes, k, d, ps = device()
            g_ms.append(ms)
            kern.append(k)
            down.append(d)
            passes.append(ps)
            digests.add(h)
        # sizes, and what the stream holds
        _, _, records, _, _ = parent(keep=True)
        _, stream, _, _, _, _ = device(keep=True)
        at, k, inflate_ok, level1 = 0, 0, True, 0
        while at < len(stream) - 28:
            size = int.from_bytes(stream[at + 16:at + 18], "little") + 1
            piece = records[k * BLOCK:(k + 1) * BLOCK]
            z = zlib.decompressobj(-15)
            inflate_ok &= z.decompress(stream[at + 18:at + size - 8]) + z.flush() == piece and z.eof
            inflate_ok &= int.from_bytes(stream[at + size - 8:at + size - 4], "little") == zlib.crc32(piece)
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            level1 += 18 + len(c.compress(piece) + c.flush()) + 8
            at += size
            k += 1
        inflate_ok &= k == (len(records) + BLOCK - 1) // BLOCK and stream[-28:] == snapgpu.bgzf_compress(b"")
        model = snapgpu.bgzf_compress_model(records)
        out.update({"G_wall_ms": _stats(g_ms), "G_kernel_ms": _stats(kern), "G_download_ms": _stats(down),
                    "G_compress_pass_ms": _stats([p[0] for p in passes]), "G_scan_ms": _stats([p[1] for p in passes]),
                    "G_gather_check_ms": _stats([p[2] for p in passes]),
                    "sha256_device": sorted(digests), "device_bytes": gbytes, "zlib6_bytes": zbytes,
                    "zlib1_bytes": level1 + 28, "blocks": k, "every_member_inflates_to_its_slice": bool(inflate_ok),
                    "device_equals_model": model == stream})
    else:
        for _ in range(reps):
            ms, z, _, nrec, zbytes = parent()
            p_ms.append(ms)
            z_ms.append(z)
    out.update({"P_wall_ms": _stats(p_ms), "P_compress_ms": _stats(z_ms), "record_bytes": nrec})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=C2["reads"])
    ap.add_argument("--genome-bases", type=int, default=C2["genome_bases"], help="a smaller genome for a quick check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "bgzf_gpu.json"))
    ap.add_argument("--child", choices=("ab", "parent"))
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be at least 3")
    if args.child:
        child(args.child, args.reps, args.reads, args.genome_bases)
        return 0

    report = {"tool": "tools/bgzf_gpu_time.py", "reps": args.reps, "reads": args.reads, "genome_bases": args.genome_bases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for name, mode, threads in (("G_and_P16", "ab", 16), ("P2", "parent", 2)):
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
    ab, p2 = report["G_and_P16"], report["P2"]
    report["G_wall_median_ms"] = ab["G_wall_ms"]["median"]
    report["P16_wall_median_ms"] = ab["P_wall_ms"]["median"]
    report["P2_wall_median_ms"] = p2["P_wall_ms"]["median"]
    report["Z16_median_ms"] = ab["P_compress_ms"]["median"]
    report["Z2_median_ms"] = p2["P_compress_ms"]["median"]
    report["device_bytes_over_zlib1_bytes"] = round(ab["device_bytes"] / ab["zlib1_bytes"], 4)
    report["device_bytes_over_zlib6_bytes"] = round(ab["device_bytes"] / ab["zlib6_bytes"], 4)
    save()
    print(f"G wall {report['G_wall_median_ms']} ms (kernels {ab['G_kernel_ms']['median']} ms), P16 {report['P16_wall_median_ms']} ms, "
          f"P2 {report['P2_wall_median_ms']} ms; device {ab['device_bytes']} B, zlib 1 {ab['zlib1_bytes']} B, zlib 6 {ab['zlib6_bytes']} B; "
          f"inflates: {ab['every_member_inflates_to_its_slice']}, equals model: {ab['device_equals_model']}", flush=True)
    return 0 if ab["every_member_inflates_to_its_slice"] and ab["device_equals_model"] else 2


if __name__ == "__main__":
    sys.exit(main())
