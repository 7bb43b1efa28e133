#!/usr/bin/env python3
"""Wall time of the seed index build, CPU builder against GPU builder, on bench.py's synthetic genomes.

For each workload (c2: chr21-sized, c3: 3.1 Gb; bench.py's genome parameters, seed length 20) the
genome is built alternately on the CPU (16 host threads, snapgpu_index_build_ex) and on the GPU
(snapgpu_index_build_gpu), `--reps` times each, every build in a process of its own.  A child
prints one JSON line: build wall seconds, the GPU builder's seconds by phase and peak device
memory, and the SHA-256 of slots and overflow.  The parent checks that every image of a workload has
the same digest, takes medians and the GPU/CPU ratio of each alternation, and writes everything to
--out (rewritten after every child, so a run that stops early leaves what it measured).

Every child runs under its own time limit and the first one that fails, faults or times out ends
the run: nothing is started on a GPU after a failure.

    python3 tools/index_build_time.py --workloads c2,c3 --reps 3 --out profiles/r07/index_build.json
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

# bench.py WORKLOADS: genome_bases, n_contigs, families; Genome.synthetic seed 2121; seed length 20
WORKLOADS = {
    "c2": dict(genome_bases=46_709_983, n_contigs=1, families=200, limit_s=180),
    "c3": dict(genome_bases=3_100_000_000, n_contigs=25, families=2000, limit_s=600),
}
SEED_LEN = 20
CPU_THREADS = 16


def _sha256(ptr, nbytes):
    h = hashlib.sha256()
    step = 1 << 30
    for off in range(0, nbytes, step):
        n = min(step, nbytes - off)
        h.update((C.c_char * n).from_address(ptr + off))
    return h.hexdigest()


def child(mode, workload, genome_bases):
    import snapgpu
    wl = WORKLOADS[workload]
    t0 = time.time()
    g = snapgpu.Genome.synthetic(genome_bases or wl["genome_bases"], seed=2121, n_contigs=wl["n_contigs"],
                                 n_repeat_families=wl["families"])
    genome_s = time.time() - t0
    if mode == "gpu":
        al = snapgpu.device_count()      # the runtime's start-up is not the build
        assert al > 0, "no HIP device"
    t1 = time.time()
    idx = snapgpu.GenomeIndex.build(g, SEED_LEN, CPU_THREADS, device=0 if mode == "gpu" else None)
    build_s = time.time() - t1
    out = {"mode": mode, "workload": workload, "genome_s": round(genome_s, 3), "build_s": round(build_s, 4)}
    if mode == "gpu":
        st = snapgpu.GenomeIndex.gpu_build_stats()
        out["phase_s"] = {k: round(v, 4) for k, v in st["phase_s"].items()}
        out["peak_device_bytes"] = st["peak_device_bytes"]
    info = idx.info()
    v = idx.view()
    t2 = time.time()
    out["sha256_slots"] = _sha256(v.slots, 12 * info["totalHashSlots"])
    out["sha256_overflow"] = _sha256(v.overflow, 4 * info["overflowTableSize"])
    out["hash_s"] = round(time.time() - t2, 2)
    out["info"] = info
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--genome-bases", type=int, default=0, help="override the workload's genome size (a quick check)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "index_build.json"))
    ap.add_argument("--child", choices=("cpu", "gpu"))
    ap.add_argument("--workload")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.workload, args.genome_bases)
        return 0

    report = {"tool": "tools/index_build_time.py", "seed_len": SEED_LEN, "cpu_threads": CPU_THREADS, "reps": args.reps,
              "workloads": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    failed = None
    for name in args.workloads.split(","):
        wl = WORKLOADS[name]
        w = report["workloads"][name] = {"genome_bases": args.genome_bases or wl["genome_bases"], "runs": []}
        for rep in range(args.reps):
            for mode in ("cpu", "gpu"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--workload", name,
                       "--genome-bases", str(args.genome_bases)]
                print(f"[{name} rep {rep} {mode}] ...", flush=True)
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=wl["limit_s"])
                    line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
                    if p.returncode != 0 or line is None:
                        failed = {"workload": name, "rep": rep, "mode": mode, "returncode": p.returncode,
                                  "stderr": p.stderr[-2000:]}
                except subprocess.TimeoutExpired:
                    failed = {"workload": name, "rep": rep, "mode": mode, "returncode": "time limit"}
                if failed:
                    break
                r = json.loads(line[len("RESULT "):])
                r["rep"] = rep
                w["runs"].append(r)
                print(f"[{name} rep {rep} {mode}] build {r['build_s']} s" +
                      (f", phases {r['phase_s']}" if mode == "gpu" else ""), flush=True)
                save()
            if failed:
                break
        cpu = [r for r in w["runs"] if r["mode"] == "cpu"]
        gpu = [r for r in w["runs"] if r["mode"] == "gpu"]
        if cpu and gpu:
            digests = {(r["sha256_slots"], r["sha256_overflow"]) for r in w["runs"]}
            w["images_equal"] = len(digests) == 1
            w["cpu_median_s"] = statistics.median(r["build_s"] for r in cpu)
            w["gpu_median_s"] = statistics.median(r["build_s"] for r in gpu)
            w["cpu_over_gpu_by_rep"] = [round(c["build_s"] / g["build_s"], 3) for c, g in zip(cpu, gpu)]
            w["cpu_over_gpu_median"] = round(w["cpu_median_s"] / w["gpu_median_s"], 3)
            w["gpu_phase_median_s"] = {k: statistics.median(r["phase_s"][k] for r in gpu) for k in gpu[0]["phase_s"]}
            w["gpu_peak_device_bytes"] = max(r["peak_device_bytes"] for r in gpu)
        if failed:
            report["stopped_at"] = failed
            save()
            print("STOPPED: " + json.dumps(failed), flush=True)
            return 1
        save()
        print(f"[{name}] images equal: {w.get('images_equal')}; CPU median {w.get('cpu_median_s')} s, "
              f"GPU median {w.get('gpu_median_s')} s", flush=True)
        if not w.get("images_equal"):
            print("IMAGES DIFFER", flush=True)
            return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
