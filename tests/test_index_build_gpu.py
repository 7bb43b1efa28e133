"""The seed index built on the GPU (snapgpu_index_build_gpu, csrc/index_build.hip) against the
CPU builder, which defines the image: every case builds one genome twice -- device=None on 4 host
threads and device=0 -- and wants equal info(), byte-equal slots / tableBase / tableSize /
overflow, and byte-equal save() files (which carry the per-table used counts).  Genomes are at
most 1 Mb."""
import os
import random

import numpy as np
import pytest

import snapgpu
from index_image import assert_same_index

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMP = str.maketrans("ACGT", "TGCA")


def _both(make_genome, seed_len, slack=0.3):
    cpu = snapgpu.GenomeIndex.build(make_genome(), seed_len, 4, slack)
    gpu = snapgpu.GenomeIndex.build(make_genome(), seed_len, slack=slack, device=0)
    return cpu, gpu


def _write_fasta(path, contigs):
    with open(path, "w") as f:
        for name, seq in contigs:
            f.write(f">{name}\n")
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
    return str(path)


def _small_world_genome():
    return snapgpu.Genome.synthetic(1_000_000, seed=2121, n_contigs=3, n_repeat_families=60)


def test_small_fa_and_reference_lookups(gpu_available, tmp_path):
    cpu, gpu = _both(lambda: snapgpu.Genome.from_fasta(os.path.join(G, "small.fa"), 500), 20)
    assert_same_index(cpu, gpu, tmp_path)
    seeds = open(os.path.join(G, "lookup_seeds.txt")).read().split()
    want = open(os.path.join(G, "expected_lookups.tsv")).read().splitlines()
    assert len(seeds) == len(want)
    for s, w in zip(seeds, want):
        f, r, (nf, nr) = gpu.lookupSeed(s)
        sums = []
        for hits in (f, r):
            acc = 0
            for h in hits:
                acc = (acc * 1000003 + h) % (1 << 64)
            sums.append(acc)
        got = f"{nf}\t{nr}\t{sums[0]}\t{sums[1]}\t{f[0] if nf else -1}\t{r[0] if nr else -1}"
        assert got == w, (s, got, w)


# 16: one table of ~1M keys, many evictions; 20: 256 tables; 25: 262,144 tables, nearly all at the
# 100-slot minimum
@pytest.mark.parametrize("seed_len", [16, 20, 25])
def test_synthetic_1mb(gpu_available, tmp_path, seed_len):
    cpu, gpu = _both(_small_world_genome, seed_len)
    im = assert_same_index(cpu, gpu, tmp_path)
    assert im["info"]["nHashTables"] == 1 << (2 * (seed_len - 16))
    assert im["info"]["totalUsedSlots"] > 500_000


@pytest.mark.parametrize("bases,slack,load", [(200_000, 0.05, 0.95), (20_000, 1e-6, 0.999)])
def test_load_near_one_linear_tail(gpu_available, tmp_path, bases, slack, load):
    """One table (seed length 16) of a repeat-free genome: nearly every seed is its own key, so the
    load is 1 / (1 + slack) -- 0.952 for 200 kb at slack 0.05.  At slack 1e-6 the table has a handful
    of free slots and most keys end up deep in the linear +1 tail of the probe sequence (20 kb there:
    a walk of that tail is one thread's chain of dependent atomics, as long as the table)."""
    cpu, gpu = _both(lambda: snapgpu.Genome.synthetic(bases, seed=77, n_contigs=1, n_repeat_families=0,
                                                      repeat_fraction=0.0, n_run_fraction=0.0), 16, slack=slack)
    im = assert_same_index(cpu, gpu, tmp_path)
    assert im["info"]["totalUsedSlots"] / im["info"]["totalHashSlots"] > load


def test_long_overflow_runs_both_sides_and_palindrome(gpu_available, tmp_path):
    rnd = random.Random(5)
    pal = "ACGGTCATGC"
    pal = pal + pal.translate(COMP)[::-1]                 # 20 bases equal to their reverse complement
    unit = pal + "".join(rnd.choice("ACGT") for _ in range(44))
    assert len(unit) == 64
    seq = unit * 2000 + unit.translate(COMP)[::-1] * 2000
    fa = _write_fasta(tmp_path / "unit.fa", [("u", seq)])
    cpu, gpu = _both(lambda: snapgpu.Genome.from_fasta(fa, 500), 20)
    assert_same_index(cpu, gpu, tmp_path)
    f, r, (nf, nr) = gpu.lookupSeed(unit[3:23], cap=8192)
    assert nf >= 1999 and nr >= 1999
    assert f == sorted(f, reverse=True) and r == sorted(r, reverse=True)
    pf, pr, (npf, npr) = gpu.lookupSeed(pal, cap=8192)
    assert npf == npr >= 3998 and pf == pr == sorted(pf, reverse=True)


def test_n_every_997_and_iupac(gpu_available, tmp_path):
    """The prime period puts a seed-run reset at every offset relative to any 64-, 256- or
    2,048-position boundary of the device passes."""
    rnd = random.Random(11)
    seq = [rnd.choice("ACGT") for _ in range(300_000)]
    for i in range(0, len(seq), 997):
        seq[i] = "N"
    for i, c in ((12_345, "R"), (150_001, "Y"), (299_990, "R")):
        seq[i] = c
    fa = _write_fasta(tmp_path / "n997.fa", [("n", "".join(seq))])
    cpu, gpu = _both(lambda: snapgpu.Genome.from_fasta(fa, 500), 20)
    im = assert_same_index(cpu, gpu, tmp_path)
    assert im["info"]["hasIupac"] == 1


def test_contig_shorter_than_seed(gpu_available, tmp_path):
    fa = _write_fasta(tmp_path / "short.fa", [("s", "ACGTACGTACGT")])
    cpu, gpu = _both(lambda: snapgpu.Genome.from_fasta(fa, 500), 20)
    im = assert_same_index(cpu, gpu, tmp_path)
    assert im["info"]["totalUsedSlots"] == 0 and im["info"]["overflowTableSize"] == 0
    assert im["info"]["totalHashSlots"] == 100 * 256


def test_alignment_over_gpu_built_index(gpu_available, small_world):
    from oracle_ffi import mismatches
    gpu_idx = snapgpu.GenomeIndex.build(_small_world_genome(), 20, device=0)
    reads = small_world["reads"]
    assert reads.n == 4000
    want = snapgpu.BaseAligner(small_world["index"], device=0).AlignReads(reads)
    got = snapgpu.BaseAligner(gpu_idx, device=0).AlignReads(reads)
    assert len(mismatches(got, want)) == 0
    assert np.array_equal(got["location"], want["location"])


def test_errors_then_a_normal_build(gpu_available, tmp_path):
    g = lambda: snapgpu.Genome.synthetic(100_000, seed=3, n_contigs=1, n_repeat_families=5)  # noqa: E731
    with pytest.raises(snapgpu.SnapGpuError) as e:
        snapgpu.GenomeIndex.build(g(), 20, device=99)
    assert "99" in str(e.value)
    with pytest.raises(snapgpu.SnapGpuError) as e:
        snapgpu.GenomeIndex.build(g(), 15, device=0)
    assert "seedLen" in str(e.value)
    cpu, gpu = _both(g, 20)
    assert_same_index(cpu, gpu, tmp_path)
    st = snapgpu.GenomeIndex.gpu_build_stats()
    assert set(st["phase_s"]) == {"upload", "scan", "sort", "runs", "sizing", "placement", "write", "download"}
    assert st["peak_device_bytes"] > 100_000 * 24
