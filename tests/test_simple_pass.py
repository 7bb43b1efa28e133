"""simple_align_kernel (csrc/simple_align.h): reads whose seeds all point at one candidate are aligned
ahead of align_kernel<128> from their pass-0 seed records; everything else bails to the general kernel.
The pass must never change a record, and it must take exactly the reads it is built for.

The genome has 120 contigs and 16 bases of padding, so the `n + MAX_K` window of a candidate at a contig
end is not servable (Genome::getSubstring searches the contig table strictly above 100 contigs, and a
window longer than the padding has to lie inside one contig).
"""
import random

import numpy as np
import pytest

import snapgpu
from oracle_ffi import mismatches, oracle_align, oracle_align_ex
from readsets import revcomp

pytestmark = pytest.mark.gpu

SEED_LEN = 20
MAX_K = 31          # LandauVishkin.h:9
N_PADDING = 100     # Genome::N_PADDING
PADDING = 16
GENOME = dict(total_bases=1_000_000, seed=41, n_contigs=120, n_repeat_families=30, repeat_fraction=0.3,
              chromosome_padding=PADDING)
N_READS = 4000


def _diff(gpu, cpu, bad, k=3):
    return "\n".join(f"read {i}\n  gpu={gpu[i]}\n  cpu={cpu[i]}" for i in bad[:k])


def _check(gpu, cpu, what=""):
    bad = mismatches(gpu, cpu)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(gpu)} differ\n" + _diff(gpu, cpu, bad)


@pytest.fixture(scope="module")
def world():
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.synthetic(**GENOME), SEED_LEN, 8)   # takes ownership of the genome
    g = snapgpu.Genome.synthetic(**GENOME)
    reads = snapgpu.Reads.synthetic(g, N_READS, seed=77, random_read_fraction=0.0)
    w = {"index": idx, "genome": g, "reads": reads, "pieces": [o for _, o in g.pieces], "n_bases": g.n_bases}
    w["oracle"] = oracle_align(idx, reads, snapgpu.default_params())
    return w


def window_ok(w, offset, length):
    """Genome::getSubstring (Genome.h:78-148) != NULL, as substring_ok of align_device.h."""
    offset, pieces, n_bases = int(offset), w["pieces"], w["n_bases"]
    if offset > n_bases or offset + length > n_bases + N_PADDING:
        return False
    if length <= PADDING:
        return True
    assert len(pieces) > 100   # (the contig table is searched strictly only above 100 contigs)
    if pieces[-1] <= offset:
        return True
    lo, hi = 0, len(pieces) - 2
    while lo <= hi:
        m = (lo + hi) // 2
        if pieces[m] <= offset:
            if pieces[m + 1] > offset:
                return not pieces[m + 1] <= offset + length - 1
            lo = m + 1
        else:
            hi = m - 1
    return False


def expected_simple(w, reads, recs):
    """-> (E, Z): the reads the simple pass must write, from the oracle's records alone.
    E is the issue's set.  Z holds the reads that met no candidate at all (nElements == 0): the pass walks
    their records to the end of the seed loop and writes their NotFound record too."""
    E, Z = [], []
    for i in range(reads.n):
        b, r = reads.get(i)[0].upper(), recs[i]
        if set(b) - set(b"ACGT") or not SEED_LEN <= len(b) <= 128:
            continue
        if r["nOverflowLists"] != 0 or r["popularSeedsSkipped"] != 0 or r["nLookups"] > 16:
            continue
        if r["nElements"] == 0 and r["nLocationsScored"] == 0:
            Z.append(i)
        # a further bail reason: the one candidate's LV call fails (its location is then invalid, so the
        # window test below says the same)
        elif (r["nElements"] == 1 and r["nLocationsScored"] == 1 and r["location"] != 0xffffffff
              and window_ok(w, r["location"], len(b) + MAX_K)):
            E.append(i)
    return E, Z


def run_both(w, reads, oracle=None, **kw):
    """The reads with the pass on and off -> (records, timing of the run with the pass on)."""
    al = snapgpu.BaseAligner(w["index"], **kw)
    on = al.AlignReads(reads)
    t_on = al.timing()
    al.set_simple_pass(False)
    off = al.AlignReads(reads)
    t_off = al.timing()
    assert on.tobytes() == off.tobytes(), f"{kw}: records differ with the pass on and off"
    assert (t_off["nSimpleReads"], t_off["nSimpleBailed"]) == (0, 0)
    cpu = oracle if oracle is not None else oracle_align(w["index"], reads, al.params)
    _check(on, cpu, str(kw))
    short = int((reads.lengths() <= 128).sum())
    assert t_on["nSimpleReads"] + t_on["nSimpleBailed"] == short, (t_on, short)
    return on, cpu, t_on


def test_on_off_bit_equality_and_oracle_parity(gpu_available, world):
    gpu, cpu, t = run_both(world, world["reads"], world["oracle"])
    print(f"nSimpleReads={t['nSimpleReads']} nSimpleBailed={t['nSimpleBailed']}")
    assert t["nSimpleReads"] > 0 and t["nSimpleBailed"] > 0


def test_coverage_from_the_oracle(gpu_available, world):
    reads, cpu = world["reads"], world["oracle"]
    E, Z = expected_simple(world, reads, cpu)
    sc = cpu["score"][E]
    assert all((sc == s).sum() >= 20 for s in (0, 1, 2)), np.bincount(sc)
    assert (cpu["nLookups"][E] > 5).sum() >= 20
    assert 0.2 * reads.n < len(E) < reads.n
    al = snapgpu.BaseAligner(world["index"])
    al.AlignReads(reads)
    t = al.timing()
    print(f"|E|={len(E)} |Z|={len(Z)} nSimpleReads={t['nSimpleReads']} nSimpleBailed={t['nSimpleBailed']}")
    assert t["nSimpleReads"] == len(E) + len(Z)


PARAM_SETS = [dict(maxK=2, extraSearchDepth=0), dict(maxK=20, maxSeedsToUse=40, extraSearchDepth=5),
              dict(maxHitsToConsider=16)]


@pytest.mark.parametrize("kw", PARAM_SETS, ids=[",".join(f"{k}={v}" for k, v in p.items()) for p in PARAM_SETS])
def test_parameter_sets(gpu_available, world, kw):
    reads = world["reads"].slice(0, 1500)
    gpu, cpu, t = run_both(world, reads, **kw)
    E, Z = expected_simple(world, reads, cpu)
    print(f"{kw}: |E|={len(E)} |Z|={len(Z)} nSimpleReads={t['nSimpleReads']} nSimpleBailed={t['nSimpleBailed']}")
    # (40 seeds to use at a limit of 25: every read needs more than the 16 records, so E is empty there)
    assert len(E) > 100 or kw.get("maxSeedsToUse", 0) > 32
    assert t["nSimpleReads"] == len(E) + len(Z), (kw, len(E), len(Z), t)


def _site(w, rng, length=128):
    """A position whose `length` bases are ACGT and which the oracle maps uniquely at every tested length."""
    g = w["genome"]
    for _ in range(200):
        p = rng.randrange(w["pieces"][3], w["pieces"][100])
        s = g.bases(p, length + 1).decode().upper()
        if set(s) - set("ACGT") or not window_ok(w, p, length + 1 + MAX_K):
            continue
        probe = snapgpu.Reads.from_list([(s[:n], "5" * n) for n in (20, 100)])
        r = oracle_align(w["index"], probe, snapgpu.default_params())
        if all(x["nElements"] == 1 and x["nLocationsScored"] == 1 and x["nOverflowLists"] == 0 and x["location"] == p
               for x in r):
            return p, s
    raise AssertionError("no uniquely mapping site")


def _sub(s, i):
    return s[:i] + ("A" if s[i] != "A" else "C") + s[i + 1:]


def test_edges(gpu_available, world):
    rng = random.Random(5)
    p, s = _site(world, rng)
    r100 = s[:100]
    cases = []   # (name, bases, the route by construction: True taken, False bailed, None a long read)
    # the first two seeds miss: the element is made by the third, with lps 2 at its creation
    cases.append(("late element", _sub(_sub(r100, 10), 30), True))
    cases.append(("reverse strand", revcomp(r100), True))
    for n in (20, 39, 60, 99, 100, 127, 128):
        cases.append((f"length {n}", s[:n], True))
    cases.append(("length 129", s[:129], None))
    cases.append(("one N", r100[:50] + "N" + r100[51:], False))
    cases.append(("indel", r100[:50] + r100[51:] + s[100], False))
    rnd = "".join(rng.choice("ACGT") for _ in range(100))
    cases.append(("matches nothing", rnd, True))
    # a repeat read with overflow lists, from the module's reads
    ovf = int(np.nonzero((world["oracle"]["nOverflowLists"] > 0) & (world["reads"].lengths() <= 128))[0][0])
    cases.append(("overflow lists", world["reads"].get(ovf)[0].decode(), False))
    # the last 100 bases of a contig that map uniquely: the candidate's window runs past the padding
    for c in range(4, 100):
        end = world["pieces"][c] - PADDING
        tail = world["genome"].bases(end - 100, 100).decode().upper()
        if set(tail) - set("ACGT"):
            continue
        o = oracle_align(world["index"], snapgpu.Reads.from_list([(tail, "5" * 100)]), snapgpu.default_params())[0]
        if o["nElements"] == 1 and o["nLocationsScored"] == 1 and o["nOverflowLists"] == 0 and o["location"] == end - 100:
            assert not window_ok(world, end - 100, 100 + MAX_K)
            cases.append(("contig end", tail, False))
            break
    assert cases[-1][0] == "contig end", "no contig with a uniquely mapping tail"
    al = snapgpu.BaseAligner(world["index"])
    for name, bases, route in cases:
        reads = snapgpu.Reads.from_list([(bases, "5" * len(bases))])
        cpu = oracle_align(world["index"], reads, al.params)
        E, Z = expected_simple(world, reads, cpu)
        if name == "late element":
            assert cpu[0]["score"] == 2 and cpu[0]["nLookups"] >= 3, cpu[0]
        if name == "matches nothing":
            assert cpu[0]["nElements"] == 0 and len(Z) == 1, cpu[0]
        if name == "overflow lists":
            assert cpu[0]["nOverflowLists"] > 0
        if name == "indel":
            assert cpu[0]["nLocationsScored"] >= 2 or cpu[0]["nElements"] >= 2, cpu[0]
        # the route by construction is the one the oracle's record implies
        assert bool(route) == (len(E) + len(Z) == 1), (name, cpu[0])
        al.set_simple_pass(True)
        gpu = al.AlignReads(reads)
        t = al.timing()
        _check(gpu, cpu, name)
        want = (0, 0) if route is None else ((1, 0) if route else (0, 1))
        assert (t["nSimpleReads"], t["nSimpleBailed"]) == want, (name, t["nSimpleReads"], t["nSimpleBailed"])
        al.set_simple_pass(False)
        assert al.AlignReads(reads).tobytes() == gpu.tobytes(), name


def test_stream_and_resident(gpu_available, world, monkeypatch):
    monkeypatch.setenv("SNAPGPU_CHUNK_READS", "700")
    reads = world["reads"]
    al = snapgpu.BaseAligner(world["index"])
    want = al.AlignReads(reads)
    tb = al.timing()
    _check(want, world["oracle"])
    out = np.zeros(reads.n, dtype=snapgpu.RESULT_DTYPE)
    al.submit(reads, out)
    al.wait()
    assert out.tobytes() == want.tobytes()
    dev = al.upload(reads)
    dev.run()
    assert dev.results().tobytes() == want.tobytes()
    tr = al.timing()
    assert (tr["nSimpleReads"], tr["nSimpleBailed"]) == (tb["nSimpleReads"], tb["nSimpleBailed"])
    assert tr["nSimpleReads"] > 0 and tb["nLaunches"] > 1   # (the blocking call ran several chunks)


def test_capped_arena(gpu_available, world, monkeypatch):
    """Reads that outgrow a 4-element arena in pass 1 still reach the big-arena pass from the list."""
    monkeypatch.setenv("SNAPGPU_ARENA_CAP", "4")
    reads = world["reads"].slice(0, 2000)
    al = snapgpu.BaseAligner(world["index"])
    gpu = al.AlignReads(reads)
    t = al.timing()
    _check(gpu, world["oracle"][:2000])
    assert t["nArenaOverflow"] > 0 and t["nSimpleReads"] > 0


def test_off_where_it_does_not_apply(gpu_available, world):
    reads = world["reads"].slice(0, 500)
    al = snapgpu.BaseAligner(world["index"], stopOnFirstHit=True)
    _check(al.AlignReads(reads), oracle_align(world["index"], reads, al.params), "stopOnFirstHit")
    t = al.timing()
    assert (t["nSimpleReads"], t["nSimpleBailed"]) == (0, 0)
    al = snapgpu.BaseAligner(world["index"])
    res, found, hits = al.AlignReadsEx(reads, None, 4)
    wres, wfound, whits = oracle_align_ex(world["index"], reads, al.params, None, 4)
    _check(res, wres, "multi-hit")
    t = al.timing()
    assert (t["nSimpleReads"], t["nSimpleBailed"]) == (0, 0)
    search = [(1000, int(world["oracle"]["location"][i]) if world["oracle"]["location"][i] != 0xffffffff else 5000,
               int(world["oracle"]["direction"][i])) for i in range(reads.n)]
    res, _, _ = al.AlignReadsEx(reads, search, 0)
    wres, _, _ = oracle_align_ex(world["index"], reads, al.params, search, 0)
    _check(res, wres, "windowed")
    t = al.timing()
    assert (t["nSimpleReads"], t["nSimpleBailed"]) == (0, 0)


def test_trip_hook_fails_the_call(gpu_available, world):
    reads = world["reads"].slice(0, 300)
    E, _ = expected_simple(world, reads, world["oracle"][:300])
    al = snapgpu.BaseAligner(world["index"])
    al.debug_trip(E[0])
    with pytest.raises(snapgpu.SnapGpuError, match=f"code 6 read {E[0]}"):
        al.AlignReads(reads)
    al.debug_trip(0xffffffff)
    _check(al.AlignReads(reads), world["oracle"][:300])
