"""Pass 0 (seed_lookup_kernel) sized to run beside the resident 128-base align kernel: one wave per
workgroup at no more than 32 VGPRs, which is what five 96-VGPR waves leave of a SIMD's 512 registers.

The records pass 0 writes must not change with the kernel's register diet, so the reads below take every
path through it and are compared with the oracle: all-ACGT reads (the table of seed offsets), reads with
an `N` (the walk over the read's used-seed bits, short and long reads, an `N` in the first seed, in the
last one and in several), reads shorter than the seed (no lookup at all) and reads of 129..150 bases (first-
round seeds of the first 128 bases, the weight, the order list).  Genome and read recipe are those of
test_lds_layout.py.  Counted on the CPU with the oracle when the recipe was written: of the 2,000 reads
72 hold an `N` (12 of them long reads), 24 are shorter than the seed, 72 have 129..150 bases; 786 end with
one element (single candidate), 846 with ten or more (repeats)."""
import numpy as np
import pytest

import snapgpu
from oracle_ffi import assert_no_corrupt_reads, mismatches, oracle_align

pytestmark = pytest.mark.gpu

GENOME = dict(total_bases=2_000_000, seed=5, n_contigs=2, n_repeat_families=12, repeat_fraction=0.7)
SEED_LEN = 20
N_READS = 2_000
LONG_LENGTHS = (129, 130, 137, 144, 149, 150)


def _with_n(read, positions):
    b, q = read
    b = bytearray(b)
    for p in positions:
        b[p % len(b)] = ord("N")
    return bytes(b), q


def build_reads(genome_kw=GENOME):
    """The 2,000 reads of the parity test (host only)."""
    g = snapgpu.Genome.synthetic(**genome_kw)
    syn = lambda n, seed, length=100: snapgpu.Reads.synthetic(g, n, seed=seed, read_length=length)
    base = syn(N_READS, 99)
    reads = []
    # 60 reads of 129..150 bases, 12 of them with an N (the long reads' walk)
    for j, length in enumerate(LONG_LENGTHS):
        part = syn(12, 200 + j, length)
        for i in range(part.n):
            r = part.get(i)
            reads.append(_with_n(r, [11 * i + j]) if i < 2 else r)
    # 60 reads of 100 bases with an N: one anywhere, in the first seed, in the last one, and three of them
    donors = syn(60, 300)
    for i in range(donors.n):
        pos = [[(7 * i) % 100], [i % SEED_LEN], [99 - i % SEED_LEN], [3 * i, 3 * i + 41, 3 * i + 77]][i % 4]
        reads.append(_with_n(donors.get(i), pos))
    # 24 reads shorter than the seed, 1..19 bases
    shorts = syn(24, 400)
    for i in range(shorts.n):
        b, q = shorts.get(i)
        n = 1 + (i * 5) % (SEED_LEN - 1)
        reads.append((b[:n], q[:n]))
    # the rest from the recipe: single-candidate and repeat reads, spread between the others
    rest = [base.get(i) for i in range(N_READS - len(reads))]
    mixed = []
    step = len(rest) // len(reads)
    for i, r in enumerate(reads):
        mixed.append(r)
        mixed += rest[i * step:(i + 1) * step]
    mixed += rest[len(reads) * step:]
    assert len(mixed) == N_READS
    return snapgpu.Reads.from_list(mixed)


def recipe_counts(reads, oracle):
    lengths = reads.lengths()
    with_n = sum(1 for i in range(reads.n) if b"N" in reads.get(i)[0])
    return {"N": with_n, "short": int((lengths < SEED_LEN).sum()),
            "long": int(((lengths >= 129) & (lengths <= 150)).sum()),
            "single": int((oracle["nElements"] == 1).sum()), "repeat": int((oracle["nElements"] >= 10).sum())}


@pytest.fixture(scope="module")
def world():
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.synthetic(**GENOME), SEED_LEN, 8)   # takes ownership of the genome
    reads = build_reads()
    return {"index": idx, "reads": reads, "oracle": oracle_align(idx, reads, snapgpu.default_params())}


def _same_as_oracle(gpu, world, what):
    assert_no_corrupt_reads(gpu)
    bad = mismatches(gpu, world["oracle"])
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(gpu)} differ from the oracle, first {bad[:5]}\n" + "\n".join(
        f"read {i}\n  gpu={gpu[i]}\n  cpu={world['oracle'][i]}" for i in bad[:3])


def test_recipe(gpu_available, world):
    c = recipe_counts(world["reads"], world["oracle"])
    print(c)
    assert world["reads"].n == N_READS
    assert c["N"] >= 50 and c["short"] >= 20 and c["long"] >= 50 and c["single"] >= 100 and c["repeat"] >= 100


def test_parity_submit_two_batches(gpu_available, world):
    """Two batches on an open stream: the second front stage is queued on the front stream while the first
    batch's align kernel runs."""
    al = snapgpu.BaseAligner(world["index"])
    half = N_READS // 2
    parts = [world["reads"].slice(0, half), world["reads"].slice(half, N_READS - half)]
    outs = [np.zeros(p.n, dtype=snapgpu.RESULT_DTYPE) for p in parts]
    for p, o in zip(parts, outs):
        al.submit(p, o)
    al.wait()
    t = al.timing()
    print(t)
    _same_as_oracle(np.concatenate(outs), world, "submit / wait")
    assert t["nLaunches"] == 2
    assert t["nSimpleReads"] > 0 and t["nSimpleBailed"] > 0


def test_parity_align_reads(gpu_available, world):
    al = snapgpu.BaseAligner(world["index"])
    gpu = al.AlignReads(world["reads"])
    t = al.timing()
    print(t)
    _same_as_oracle(gpu, world, "AlignReads")
    assert t["nSimpleReads"] > 0 and t["nSimpleBailed"] > 0


def test_parity_without_simple_pass(gpu_available, world, monkeypatch):
    """SNAPGPU_SIMPLE_PASS=0: align_kernel<128> consumes pass 0's records of every read."""
    monkeypatch.setenv("SNAPGPU_SIMPLE_PASS", "0")
    al = snapgpu.BaseAligner(world["index"])
    gpu = al.AlignReads(world["reads"])
    t = al.timing()
    _same_as_oracle(gpu, world, "SNAPGPU_SIMPLE_PASS=0")
    assert (t["nSimpleReads"], t["nSimpleBailed"]) == (0, 0)


def test_pass0_fits_beside_the_align_kernel(gpu_available, world):
    """Five align_kernel<128> waves and one pass-0 wave fit a SIMD's 512 VGPRs; 20 align waves per CU."""
    g = snapgpu.BaseAligner(world["index"]).debug_grids()
    print(g)
    assert g["vgprLookup"] <= 32
    assert 5 * g["vgpr128"] + g["vgprLookup"] <= 512
    assert g["perCU128"] == 20
