"""The seed path of align_kernel<128> around the scorer: seeds whose hits change nothing, score calls
that find no linked element, singleton seeds (no overflow list in either direction), the wrap of the
seed sequence (the lps quotient by a reciprocal, small_div.h) and the one-element non-forced pop on
both sides of its 64-element shortcut.  Every record field is compared with the oracle.
"""
import os
import random
import subprocess

import numpy as np
import pytest

import snapgpu
from oracle_ffi import mismatches, oracle_align, oracle_align_ex
from readsets import revcomp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SEED_LEN = 20
UNIQUE = dict(total_bases=1_000_000, seed=31, n_contigs=2, n_repeat_families=0, repeat_fraction=0.0)
# a few long-lived families: a read inside one has from a handful to several hundred candidate elements
REPEAT = dict(total_bases=2_000_000, seed=5, n_contigs=2, n_repeat_families=12, repeat_fraction=0.7)


def _diff(gpu, cpu, bad, k=3):
    return "\n".join(f"read {i}\n  gpu={gpu[i]}\n  cpu={cpu[i]}" for i in bad[:k])


def _check(gpu, cpu, what=""):
    bad = mismatches(gpu, cpu)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(gpu)} differ\n" + _diff(gpu, cpu, bad)


def _world(spec):
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.synthetic(**spec), SEED_LEN, 8)   # takes ownership of the genome
    return {"index": idx, "genome": snapgpu.Genome.synthetic(**spec)}


@pytest.fixture(scope="module")
def unique():
    return _world(UNIQUE)


@pytest.fixture(scope="module")
def repeat():
    w = _world(REPEAT)
    w["reads"] = snapgpu.Reads.synthetic(w["genome"], 4000, seed=17)
    return w


def seed_window_reads(genome, n_reads, seed=3):
    """Error-free 100-base reads with one substitution in the middle of 1..4 of the first round's five
    seed windows (offsets 0, 20, .., 80), half of them reverse-complemented: those seeds are applied
    with zero hits (the mutated 20-mer is absent from a repeat-free genome)."""
    rng = random.Random(seed)
    out = []
    while len(out) < n_reads:
        p = rng.randrange(1000, genome.n_bases - 1200)
        s = genome.bases(p, 100).decode().upper()
        if set(s) - set("ACGT"):
            continue
        t = list(s)
        for w in rng.sample(range(5), rng.randrange(1, 5)):
            i = w * SEED_LEN + rng.randrange(6, 14)
            t[i] = rng.choice([b for b in "ACGT" if b != t[i]])
        t = "".join(t)
        out.append((revcomp(t) if rng.random() < 0.5 else t, "2" * 100))
    return snapgpu.Reads.from_list(out)


@pytest.mark.gpu
def test_error_free_reads_of_a_repeat_free_genome(gpu_available, unique):
    """Every seed after a read's first hits the candidate that is scored already, and the score call
    after it finds nothing linked."""
    reads = snapgpu.Reads.synthetic(unique["genome"], 3000, seed=11, base_error_rate=0.0, mutation_rate=0.0)
    al = snapgpu.BaseAligner(unique["index"])
    gpu = al.AlignReads(reads)
    _check(gpu, oracle_align(unique["index"], reads, al.params))
    assert (gpu["result"] == snapgpu.SingleHit).sum() > 2500
    assert np.median(gpu["nElements"]) <= 2


@pytest.mark.gpu
def test_substitutions_inside_seed_windows(gpu_available, unique):
    reads = seed_window_reads(unique["genome"], 3000)
    al = snapgpu.BaseAligner(unique["index"])
    gpu = al.AlignReads(reads)
    _check(gpu, oracle_align(unique["index"], reads, al.params))
    # a seed with zero hits is still looked up: more lookups than hit words
    assert (gpu["nLookups"] > gpu["nHitWords"]).sum() > 1500


WRAP_SETS = [dict(read_length=40), dict(read_length=100, maxSeedsToUse=60), dict(read_length=100, maxSeedsToUse=200)]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", WRAP_SETS, ids=[",".join(f"{k}={v}" for k, v in p.items()) for p in WRAP_SETS])
def test_seed_sequence_wraps(gpu_available, repeat, kw):
    """40-base reads have two seeds per round and 25 seeds to use: the sequence wraps and
    mostSeedsContainingAnyParticularBase rises past 1; 100-base reads wrap with more seeds to use.  Random
    reads (no hit ends them early) run the sequence to its end."""
    kw = dict(kw)
    n = kw.pop("read_length")
    reads = snapgpu.Reads.synthetic(repeat["genome"], 3000, seed=23, read_length=n, random_read_fraction=0.1)
    al = snapgpu.BaseAligner(repeat["index"], **kw)
    gpu = al.AlignReads(reads)
    _check(gpu, oracle_align(repeat["index"], reads, al.params), str(kw))
    per_round = (n - SEED_LEN) // SEED_LEN + 1
    assert (gpu["nLookups"] > per_round).sum() > 100, "no read wrapped"


def _mixed_seed(index, reads, n_scan=400):
    """A first-round seed of the reads with one hit in one direction and an overflow list in the other."""
    for i in range(min(n_scan, reads.n)):
        b = reads.get(i)[0].upper()
        for o in range(0, len(b) - SEED_LEN + 1, SEED_LEN):
            s = b[o:o + SEED_LEN]
            if set(s) - set(b"ACGT"):
                continue
            _, _, (nf, nr) = index.lookupSeed(s, cap=4)
            if (nf == 1 and nr > 1) or (nr == 1 and nf > 1):
                return i, o, nf, nr
    return None


@pytest.mark.gpu
def test_repeat_families_at_1000_hits(gpu_available, repeat):
    """Reads of repeat families at maxHitsToConsider 1000: few-element reads, both sides of the 64-element
    shortcut of the non-forced pop, and of the LDS caps (192 mirrored elements and selection keys)."""
    reads = repeat["reads"]
    al = snapgpu.BaseAligner(repeat["index"], maxHitsToConsider=1000)
    gpu = al.AlignReads(reads)
    _check(gpu, oracle_align(repeat["index"], reads, al.params))
    ne = gpu["nElements"]
    bins = {"1..5": ((ne >= 1) & (ne <= 5)).sum(), "6..64": ((ne >= 6) & (ne <= 64)).sum(),
            "65..192": ((ne >= 65) & (ne <= 192)).sum(), ">192": (ne > 192).sum()}
    print(bins)
    assert all(v >= 20 for v in bins.values()), bins
    assert _mixed_seed(repeat["index"], reads) is not None, "no seed with a singleton and a list"


@pytest.mark.gpu
def test_multihit_twin(gpu_available, repeat, unique):
    """align_kernel<128, true> (AlignReads_ex with multi-hit export) over the same reads."""
    for w, reads, kw in ((repeat, repeat["reads"].slice(0, 2500), dict(maxHitsToConsider=1000)),
                         (unique, seed_window_reads(unique["genome"], 1500), {})):
        al = snapgpu.BaseAligner(w["index"], **kw)
        res, found, hits = al.AlignReadsEx(reads, None, 8)
        wres, wfound, whits = oracle_align_ex(w["index"], reads, al.params, None, 8)
        _check(res, wres, str(kw))
        assert np.array_equal(found, wfound)
        for i in np.nonzero(wfound > 0)[0]:
            assert np.array_equal(hits[i, :wfound[i]], whits[i, :wfound[i]]), i


@pytest.mark.gpu
def test_stream_equals_resident(gpu_available, repeat):
    al = snapgpu.BaseAligner(repeat["index"], maxHitsToConsider=1000)
    stream = al.AlignReads(repeat["reads"])
    dev = al.upload(repeat["reads"])
    dev.run()
    resident = dev.results()
    assert np.array_equal(stream.view(np.uint8), resident.view(np.uint8))


def test_quotient_by_reciprocal_equals_division(tmp_path):
    """small_div.h on the host: every dividend 0..512 and divisor 1..32 (tests/c/small_div_test.cpp)."""
    exe = tmp_path / "small_div_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "snap-rnaseq_amd", "csrc"),
                    os.path.join(HERE, "c", "small_div_test.cpp"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "16416 pairs, 0 mismatches" in out.stdout, out.stdout[-2000:]
