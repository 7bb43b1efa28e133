"""The four-reads-per-wave path of simple_align_kernel (csrc/simple_align.h, simple_quad): read g of a quad in
lanes 16g .. 16g+15, the seed walk as per-lane predicates over the walk schedule, one narrow LV pass (limit 7)
for all four, and simple_one as the one-read path for whatever the quad path hands on.

Every case checks the records against the oracle, byte equality with the pass switched off, and
nSimpleReads + nSimpleBailed == the reads of at most 128 bases (run_both of test_simple_pass.py).  nSimpleWide
counts the records the one-read path wrote: without it a build that sent every read there would pass.
The genome is test_simple_pass.py's (1 Mb, 120 contigs, padding 16)."""
import itertools
import random

import numpy as np
import pytest

import snapgpu
from oracle_ffi import oracle_align
from test_simple_pass import _check, _site, _sub, expected_simple, run_both, world  # noqa: F401  (world: fixture)

pytestmark = pytest.mark.gpu

COUNTERS = ("nSimpleReads", "nSimpleBailed", "nSimpleWide")


def _reads(seqs):
    return snapgpu.Reads.from_list([(s, "5" * len(s)) for s in seqs])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 31, 32, 33, 63, 65])
def test_batch_sizes(gpu_available, world, n):
    """Partial quads and partial 32-read chunks: prefixes of the module's reads."""
    gpu, cpu, t = run_both(world, world["reads"].slice(0, n), world["oracle"][:n])
    E, Z = expected_simple(world, world["reads"].slice(0, n), cpu)
    print(f"n={n}: |E|={len(E)} |Z|={len(Z)} " + " ".join(f"{c}={t[c]}" for c in COUNTERS))
    assert t["nSimpleReads"] == len(E) + len(Z)
    assert t["nSimpleWide"] <= t["nSimpleReads"]


def test_mixed_quads(gpu_available, world):
    """A uniquely mapping read, an overflow-list read, a 129-base read and a read with one N, in all 24 orders:
    each kind in each group position, next to each other kind."""
    rng = random.Random(11)
    p, s = _site(world, rng)
    r100 = s[:100]
    ovf = int(np.nonzero((world["oracle"]["nOverflowLists"] > 0) & (world["reads"].lengths() <= 128))[0][0])
    kinds = [r100, world["reads"].get(ovf)[0].decode(), s[:129], r100[:50] + "N" + r100[51:]]
    seqs = [kinds[i] for order in itertools.permutations(range(4)) for i in order]
    assert len(seqs) == 96
    reads = _reads(seqs)
    gpu, cpu, t = run_both(world, reads)
    print(" ".join(f"{c}={t[c]}" for c in COUNTERS))
    one = oracle_align(world["index"], _reads(kinds), snapgpu.default_params())
    assert one[0]["nElements"] == 1 and one[0]["nLocationsScored"] == 1 and one[1]["nOverflowLists"] > 0
    # the unique read is written by the quad path, the overflow read bails in it; the N read goes through the
    # one-read path, which bails on the N; the long read is pass 2's
    assert (t["nSimpleReads"], t["nSimpleBailed"], t["nSimpleWide"]) == (24, 48, 0)


def _narrow_cases(s):
    """(name, read, intended score): substitutions around a clean linking seed of the 100-base site s.  The
    seed sequence of a 100-base read starts 0, 20, 40, 60, 80; the first clean seed links."""
    def subs(pos):
        r = s[:100]
        for i in pos:
            r = _sub(r, i)
        return r
    return [
        ("7 after the seed", subs([25, 35, 45, 55, 65, 75, 85]), 7),
        ("7 before the seed", subs([5, 15, 25, 35, 45, 55, 65]), 7),
        ("3 + 4", subs([5, 25, 35, 65, 75, 85, 95]), 7),
        ("4 + 4", subs([5, 15, 25, 35, 65, 75, 85, 95]), 8),
        ("8 + 0", subs([22, 32, 42, 52, 62, 72, 82, 92]), 8),
        ("0 + 8", subs([5, 15, 25, 35, 45, 55, 65, 75]), 8),
        ("14", subs([22 + 5 * i for i in range(14)]), 14),
        ("15", subs([22 + 5 * i for i in range(15)]), 15),
    ]


def test_narrow_limit(gpu_available, world):
    """Scores up to 7 are the quad path's; 8 and above are still the pass's, through the one-read path: a
    failure of the narrow LV pass never bails by itself."""
    rng = random.Random(23)
    p, s = _site(world, rng)
    al = snapgpu.BaseAligner(world["index"])
    kept = []
    for name, bases, score in _narrow_cases(s):
        reads = _reads([bases])
        cpu = oracle_align(world["index"], reads, al.params)
        o = cpu[0]
        if not (o["nElements"] == 1 and o["nLocationsScored"] == 1 and o["nOverflowLists"] == 0
                and o["score"] == score and o["location"] == p):
            print(f"{name}: the oracle maps it otherwise, not used: {o}")
            continue
        kept.append(score)
        al.set_simple_pass(True)
        gpu = al.AlignReads(reads)
        t = al.timing()
        print(f"{name}: score {o['score']} nLookups {o['nLookups']} " + " ".join(f"{c}={t[c]}" for c in COUNTERS))
        _check(gpu, cpu, name)
        assert (t["nSimpleReads"], t["nSimpleBailed"]) == (1, 0), (name, t)
        assert t["nSimpleWide"] == (1 if score >= 8 else 0), (name, t)
        al.set_simple_pass(False)
        assert al.AlignReads(reads).tobytes() == gpu.tobytes(), name
    assert min(kept) <= 7 and max(kept) >= 8 and len(kept) >= 6, kept


def _acgt_only(reads, n):
    out = []
    for i in range(reads.n):
        b, q = reads.get(i)
        if not set(b.upper()) - set(b"ACGT"):
            out.append((b.decode(), q.decode()))
        if len(out) == n:
            break
    return snapgpu.Reads.from_list(out)


def test_narrow_pass_is_the_whole_pass(gpu_available, world):
    """maxK 2, extraSearchDepth 0: the first limit is 2, so the narrow LV pass is simple_one's."""
    reads = _acgt_only(world["reads"], 1500)
    gpu, cpu, t = run_both(world, reads, maxK=2, extraSearchDepth=0)
    E, Z = expected_simple(world, reads, cpu)
    print(f"|E|={len(E)} |Z|={len(Z)} " + " ".join(f"{c}={t[c]}" for c in COUNTERS))
    assert len(E) > 100 and t["nSimpleReads"] == len(E) + len(Z)
    assert t["nSimpleWide"] == 0


def test_seventeenth_record(gpu_available, world):
    """maxK 20, 40 seeds, extraSearchDepth 5: no limit ends the walk within 16 records, so everything bails."""
    reads = world["reads"].slice(0, 1500)
    gpu, cpu, t = run_both(world, reads, maxK=20, maxSeedsToUse=40, extraSearchDepth=5)
    short = int((reads.lengths() <= 128).sum())
    assert (t["nSimpleReads"], t["nSimpleBailed"], t["nSimpleWide"]) == (0, short, 0)


def test_max_hits_16(gpu_available, world):
    reads = world["reads"].slice(0, 1500)
    gpu, cpu, t = run_both(world, reads, maxHitsToConsider=16)
    E, Z = expected_simple(world, reads, cpu)
    print(f"|E|={len(E)} |Z|={len(Z)} " + " ".join(f"{c}={t[c]}" for c in COUNTERS))
    assert t["nSimpleReads"] == len(E) + len(Z)


def test_the_fast_path_is_the_path(gpu_available, world):
    reads, cpu = world["reads"], world["oracle"]
    E, Z = expected_simple(world, reads, cpu)
    low = int((cpu["score"][E] <= 7).sum()) + len(Z)
    print(f"|E|={len(E)} |Z|={len(Z)} score <= 7 or no candidate: {low}")
    assert low >= 0.97 * (len(E) + len(Z))   # the precondition, from the oracle's records
    al = snapgpu.BaseAligner(world["index"])
    _check(al.AlignReads(reads), cpu)
    t = al.timing()
    print(" ".join(f"{c}={t[c]}" for c in COUNTERS))
    assert t["nSimpleReads"] == len(E) + len(Z)
    # a cap that keeps the one-read path from hiding a dead quad path, not a measurement
    assert t["nSimpleWide"] <= 0.05 * t["nSimpleReads"]


def test_chunked_stream_and_resident(gpu_available, world, monkeypatch):
    monkeypatch.setenv("SNAPGPU_CHUNK_READS", "700")
    reads = world["reads"]
    al = snapgpu.BaseAligner(world["index"])
    want = al.AlignReads(reads)
    tb = al.timing()
    _check(want, world["oracle"])
    assert tb["nLaunches"] > 1 and tb["nSimpleReads"] > 0
    out = np.zeros(reads.n, dtype=snapgpu.RESULT_DTYPE)
    al.submit(reads, out)
    al.wait()
    ts = al.timing()
    assert out.tobytes() == want.tobytes()
    dev = al.upload(reads)
    dev.run()
    assert dev.results().tobytes() == want.tobytes()
    tr = al.timing()
    for t in (ts, tr):
        assert tuple(t[c] for c in COUNTERS) == tuple(tb[c] for c in COUNTERS), (t, tb)
