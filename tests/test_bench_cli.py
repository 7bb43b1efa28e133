"""bench.py's command line: a plain run times the steps and prints the line, `--full` adds the legs
that take runs of their own, `--dump-outputs DIR` writes the last timed step's records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("resident", "lookup_roofline", "copy_peak", "sam_records", "paired", "single_e2e", "rna_paired")


def _records(n, seed=3):
    import snapgpu
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=snapgpu.RESULT_DTYPE)
    res["location"] = rng.integers(0, 2**32, n, dtype=np.uint64)
    res["score"] = rng.integers(-1, 15, n)
    res["mapq"] = rng.integers(0, 71, n)
    res["result"] = rng.integers(0, 3, n)
    res["nLocationsScored"] = rng.integers(0, 20000, n)
    res["probabilityOfAllCandidates"] = rng.random(n)
    res["probabilityOfBestCandidate"] = rng.random(n) * 1e-30
    return res


def test_dump_outputs_holds_every_record_exactly(tmp_path):
    import bench
    res = _records(5000)
    assert bench.dump_outputs(str(tmp_path / "d"), res) == 5000
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == sorted(name + ".npy" for name, _ in bench.DUMP_FIELDS)
    for name, t in bench.DUMP_FIELDS:
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == t and a.dtype in (np.float32, np.float64) and a.shape == (5000,)
        assert np.array_equal(a.astype(res.dtype[name]), res[name]), name   # no value rounded by the float type


def test_dump_outputs_samples_a_large_batch_within_the_cap(tmp_path):
    import bench
    per_record = sum(np.dtype(t).itemsize for _, t in bench.DUMP_FIELDS)
    n = bench.DUMP_MAX_BYTES // per_record + 1000     # the smallest kind of batch that no longer fits
    res = _records(n)
    kept = [bench.dump_outputs(str(tmp_path / d), res) for d in ("a", "b")]
    assert kept[0] == kept[1] < n
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES
    sel = np.load(tmp_path / "a" / "sample_index.npy")
    assert np.array_equal(sel, np.load(tmp_path / "b" / "sample_index.npy"))    # the same sample every run
    idx = sel.astype(np.int64)
    assert len(idx) == kept[0] and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "location.npy").astype(np.uint32), res["location"][idx])


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", "3000", "--genome-bases", "400000",
           *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_steps_records(gpu_available, tmp_path):
    """--steps 1 and --steps 3 both run (one and three timed steps), print the headline without the
    legs of --full, and dump the same records: those of a direct AlignReads on the same inputs."""
    import bench
    import snapgpu
    d1 = _bench("--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "s1"))
    d3 = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "s3"))
    for d, steps in ((d1, 1), (d3, 3)):
        assert all(k in d for k in HEADLINE) and d["steps"] == steps
        assert d["value"] == pytest.approx(3000 * steps / (d["ms_per_step"] * steps / 1000.0), rel=1e-6)
        assert not any(k in d for k in FULL_ONLY) and d["cpu_baseline"] is None and d["parity"] is None
    wl = bench.WORKLOADS["c2"]
    g = snapgpu.Genome.synthetic(400_000, seed=2121, n_contigs=wl["n_contigs"], n_repeat_families=wl["families"])
    idx = snapgpu.GenomeIndex.build(g, 20, 4)
    reads = snapgpu.Reads.synthetic(idx.genome_handle(), 3000, seed=99)
    want = snapgpu.BaseAligner(idx, device=0).AlignReads(reads)
    assert (want["result"] == snapgpu.SingleHit).sum() > 2000
    for name, t in bench.DUMP_FIELDS:
        a, b = np.load(tmp_path / "s1" / (name + ".npy")), np.load(tmp_path / "s3" / (name + ".npy"))
        assert a.dtype == t and np.array_equal(a, b), name
        assert np.array_equal(a.astype(want.dtype[name]), want[name]), name


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(gpu_available):
    d = _bench("--full", "--steps", "2", "--warmup", "1", "--paired-pairs", "2000", "--single-reads", "0",
               "--rna-pairs", "0", "--cpu-sample", "3000")
    assert all(k in d for k in HEADLINE)
    assert d["parity"] == dict(d["parity"], reads_compared=3000, mismatches=0)
    assert d["cpu_baseline"]["value"] > 0 and d["resident"]["same_results"]
    assert d["paired"]["parity"]["mismatches"] == 0 and d["sam_records"]["parity"]["mismatches"] == 0
