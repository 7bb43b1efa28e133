"""The paired aligner outside the slice test_paired.py covers (one genome at seed length 20, equal mates of
at most 150 bases, command-line seed counts): PAIRED_EDGE_SETS of golden_common.py, every set pinned
bitwise to the reference's own rows (`ref_harness paired`, tests/golden/make_golden.py --only-paired-edges).

* long_default / long_wide -- small.fa; each mate's length drawn on its own from 49..500, so L0 != L1 is the
  rule: reads of 257..500 bases in a pair (host list -> pass 1b -> defer -> pass 2, PLds<512> with byte
  compares), mates of different lengths (60 + 400, 128 + 129, 256 + 257: the host routes by max(L0, L1),
  `more` / `fewer` and the pair's seed count depend on both), the chimeric fallback above 256 bases,
  pairs over the genome's IUPAC bytes, pairs at both ends of a contig.
* tandem -- tandem.fa, 300 copies of a 20-base unit, maxSpacing 3000: more than 64 and more than 128 mates
  inside one spacing window, so the scan for the lowest best-possible score takes two and three steps.
* repeat_default / repeat_wide -- repeat.fa (1,800 copies of one element): hits by the thousand against the
  pass-1 pools; under `wide`, maxBigHits 64 skips the popular seeds and they enter the MAPQ.
* seed16 / seed25 -- small.fa indexed at seed lengths 16 and 25, the first 600 pairs of paired_{1,2}.fq.
* coverage -- maxSeedsToUse 0, seedCoverage 2.0: seeds per pair = max(L0, L1) * seedCoverage / seedLen.

CPU: the C restatement (oracle/snap_oracle.c) equals the reference's rows, both aligners.
GPU: snapgpu_paired_intersect_batch / snapgpu_paired_align_batch equal the reference's rows and the
restatement; the pass that wrote each record (`writtenBy`) follows the routing rules; one wave aligning the
`long` pairs in a row equals the full grid; SNAPGPU_PFLAG_POOL_EXHAUSTED is raised for the pairs the
restatement flags and for no other.
"""
import os

import numpy as np
import pytest

import snapgpu
from snapgpu import _ffi as F
from golden_common import PAIRED_EDGE_FIRST, PAIRED_EDGE_MAXLEN, PAIRED_EDGE_SETS, golden_path
from oracle_ffi import oracle_paired, paired_tsv_rows, ref_paired_rows
from test_paired import _bitwise, _cmp, _dump_failure, _no_corrupt_reads

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")

# the field list of test_paired.py's test_gpu_intersecting_matches_reference_and_oracle
FIELDS = ("status", "location", "direction", "score", "mapq", "nLocationsScored", "popularSeedsSkipped",
          "probabilityOfAllPairs", "probabilityOfBestPair")
SNAPGPU_EINVAL = -1   # include/snapgpu.h

_indexes, _reads, _oracle = {}, {}, {}


def _index(fa, seed_len):
    if (fa, seed_len) not in _indexes:
        _indexes[fa, seed_len] = snapgpu.GenomeIndex.build(snapgpu.Genome.from_fasta(golden_path(fa), 500),
                                                           seed_len, 4)
    return _indexes[fa, seed_len]


def _world(name):
    """(index, reads0, reads1, parameters) of a set; indexes and read batches are shared between the tests."""
    fa, seed_len, stem, p = PAIRED_EDGE_SETS[name]
    key = (stem, PAIRED_EDGE_FIRST.get(name), PAIRED_EDGE_MAXLEN.get(name))
    if key not in _reads:
        r = [snapgpu.Reads.from_fastq(golden_path(f"{stem}_{k}.fq")) for k in (1, 2)]
        if key[1]:
            r = [x.slice(0, key[1]) for x in r]
        if key[2]:   # the pairs with both mates of at most that many bases
            keep = np.nonzero(np.maximum(r[0].lengths(), r[1].lengths()) <= key[2])[0]
            r = [snapgpu.Reads.from_list([x.get(int(i)) for i in keep]) for x in r]
        assert r[0].n == r[1].n <= 600
        _reads[key] = r
    return _index(fa, seed_len), _reads[key][0], _reads[key][1], p


def _kwargs(p, **over):
    kw = dict(maxHits=p["maxHits"], maxK=p["maxK"], maxSeedsToUse=p["numSeeds"], extraSearchDepth=p["extra"],
              minSpacing=p["minSpacing"], maxSpacing=p["maxSpacing"], maxBigHits=p["maxBigHits"],
              seedCoverage=p.get("seedCoverage", 0.0))
    kw.update(over)
    return kw


def _params(p, **over):
    q = F.PairedParams()
    for k, v in {**dict(maxCandidatePoolSize=1000000, maxReadSize=500, forceSpacing=0), **_kwargs(p, **over)}.items():
        setattr(q, k, v)
    return q


def _restatement(name, chimeric):
    """The restatement's records of a set, computed once and left unchanged."""
    if (name, chimeric) not in _oracle:
        idx, r0, r1, p = _world(name)
        res = oracle_paired(idx, r0, r1, _params(p), chimeric=chimeric)
        res.setflags(write=False)
        _oracle[name, chimeric] = res
    return _oracle[name, chimeric]


def _want(name):
    return ref_paired_rows(golden_path(f"expected_paired_edge_{name}.tsv"))


def _has_other(reads, i):
    """Read i holds a byte outside ACGTN (either case)."""
    return bool(set(reads.get(i)[0].upper()) - set(b"ACGTN"))


# ------------------------------------------------------------------------- CPU
def test_edge_fixture_shapes():
    """What the generator asserted when it wrote the sets, again from the committed files: the length
    classes of `long`, its IUPAC pairs (counted, not there by chance), mates of 100 bases elsewhere."""
    _, r0, r1, _ = _world("long_default")
    l0, l1 = r0.lengths().astype(int), r1.lengths().astype(int)
    mx, mn = np.maximum(l0, l1), np.minimum(l0, l1)
    assert (mx <= 128).sum() >= 20 and ((mx >= 129) & (mx <= 256)).sum() >= 20 and (mx >= 257).sum() >= 20
    assert ((mn <= 128) & (mx > 256)).sum() >= 20
    assert ((l0 == 500) | (l1 == 500)).sum() >= 10 and ((l0 == 49) | (l1 == 49)).sum() >= 10
    assert mx.max() == 500 and (mx < 50).sum() >= 1
    assert ((l0 != l1) & (mn >= 50)).sum() >= 200          # mates of different lengths, both aligned
    for a, b in ((60, 400), (128, 129), (256, 257)):       # across each routing threshold
        assert (((mn <= a) & (mx >= b)) & (mn >= 50)).sum() >= 5, (a, b)
    iupac = [i for i in range(r0.n) if _has_other(r0, i) or _has_other(r1, i)]
    assert len(iupac) >= 15
    assert sum(1 for i in iupac if mn[i] >= 50 and mx[i] <= 256) >= 5
    _, c0, c1, cp = _world("coverage")
    cm = np.maximum(c0.lengths(), c1.lengths()).astype(int)
    # no pair asks for more seeds than the reference's MAX_MAX_SEEDS, and the count does vary with the pair
    seeds = (cm * cp["seedCoverage"] / 20).astype(int)
    assert cm.max() <= 256 and seeds.max() <= 30 and len(set(seeds)) >= 5 and cp["numSeeds"] == 0
    for name in ("tandem", "repeat_default"):
        _, t0, t1, _ = _world(name)
        assert (t0.lengths() == 100).all() and (t1.lengths() == 100).all() and t0.n >= 80


@pytest.mark.parametrize("name", list(PAIRED_EDGE_SETS))
def test_oracle_paired_edges_match_reference(name):
    """The restatement against the reference's rows on every set and run, the intersecting aligner alone
    and the chimeric one (above 256 bases this is the first pin of either to the reference, and of the
    single-end fallback inside a pair; seed lengths 16 and 25 and the seedCoverage seed count
    (maxSeedsToUse 0) were pinned for pairs nowhere)."""
    inter_want, chim_want = _want(name)
    bad = _cmp(paired_tsv_rows(_restatement(name, False), chimeric=False), inter_want)
    assert not bad, f"intersecting: {len(bad)} pairs differ, first {bad[:3]}"
    bad = _cmp(paired_tsv_rows(_restatement(name, True), chimeric=True), chim_want)
    assert not bad, f"chimeric: {len(bad)} pairs differ, first {bad[:3]}"


def test_edge_outcome_mix():
    """The sets reach the branches they were built for, by the reference's own rows: `long` aligns pairs
    together, through the fallback and not at all; under `wide` the repeat pairs differ from `default`
    (maxBigHits 64 biting) and the restatement reports skipped popular seeds there."""
    chim = [row.split("\t") for row in _want("long_default")[1]]
    together = sum(1 for c in chim if c[10] == "1")
    fallback = sum(1 for c in chim if c[10] == "0" and c[0] != "0")
    untouched = sum(1 for c in chim if c[0] == "0" and c[1] == "0" and c[2] == str(0xFFFFFFFF))
    assert together >= 100 and fallback >= 20 and untouched >= 10
    d, w = _want("repeat_default")[0], _want("repeat_wide")[0]
    assert sum(1 for a, b in zip(d, w) if a != b) >= 20
    assert (_restatement("repeat_wide", False)["popularSeedsSkipped"] > 0).sum() >= 20
    assert (_restatement("repeat_default", False)["popularSeedsSkipped"] == 0).all()


# Pool exhaustion: maxCandidatePoolSize for the `repeat` pairs.  The reference's pool is min(this,
# maxBigHits * seeds * 2) entries, half of it per set pair for the mates.  A pair with both mates inside
# element copies collects a mate per copy in reach of a hit of the other read, several hundred of them; a
# pair with one mate in a contig's random head collects a handful.  At 400 entries the restatement flags
# the first kind and completes the second (asserted below, on the CPU).
EXHAUST_POOL = 400


def _exhausted_restatement():
    if "exhaust" not in _oracle:
        idx, r0, r1, p = _world("repeat_default")
        res = oracle_paired(idx, r0, r1, _params(p, maxCandidatePoolSize=EXHAUST_POOL), chimeric=False)
        res.setflags(write=False)
        _oracle["exhaust"] = res
    return _oracle["exhaust"]


def test_oracle_pool_exhaustion_is_partial():
    """The restatement under EXHAUST_POOL flags at least 10 and fewer than all of the repeat pairs
    (snap_oracle.c: the three `Ran out of ... pool entries` sites), and returns the records: the flags are
    the data.  Unflagged pairs are the default pool's records (the pool size changes nothing else)."""
    cpu = _exhausted_restatement()
    flagged = (cpu["flags"] & snapgpu.PFLAG_POOL_EXHAUSTED) != 0
    assert 10 <= int(flagged.sum()) < len(cpu) - 10, int(flagged.sum())
    full = _restatement("repeat_default", False)
    assert len(_bitwise(cpu[~flagged], full[~flagged], FIELDS)) == 0


# ------------------------------------------------------------------------- GPU
def _aligner(name, **over):
    idx, _, _, p = _world(name)
    return snapgpu.PairedAligner(idx, **_kwargs(p, **over))


@pytest.fixture(scope="module")
def gpu_runs(gpu_available):
    """intersect() and align() of a fresh aligner per set, run once and shared (default pools, no hook)."""
    cache = {}

    def get(name):
        if name not in cache:
            _, r0, r1, _ = _world(name)
            pa = _aligner(name)
            inter, chim = pa.intersect(r0, r1), pa.align(r0, r1)
            for x in (inter, chim):
                x.setflags(write=False)
            cache[name] = (inter, chim)
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PAIRED_EDGE_SETS))
def test_gpu_paired_edges_match_reference_and_oracle(gpu_runs, name):
    """Parity on every set and run: intersect and align equal the reference's rows, and intersect equals
    the restatement bitwise, the two probabilities included.  Closes, per set: reads of 257..500 bases in
    a pair and mates of different lengths (long_*), the chimeric fallback above 256 bases (long_*, align),
    more than 64 mates in one spacing window (tandem), repeats for pairs and maxBigHits skipping with
    popularSeedsSkipped in the MAPQ (repeat_*), seed lengths 16 and 25, and maxSeedsToUse == 0."""
    _, r0, r1, _ = _world(name)
    inter, chim = gpu_runs(name)
    _no_corrupt_reads(inter)
    _no_corrupt_reads(chim)
    inter_want, chim_want = _want(name)
    bad = _cmp(paired_tsv_rows(inter, chimeric=False), inter_want)
    if bad:
        _dump_failure(f"edge_intersect_{name}", inter, bad, r0, r1)
    assert not bad, f"intersect: {len(bad)} pairs differ from the reference, first {bad[:3]}"
    bad = _cmp(paired_tsv_rows(chim, chimeric=True), chim_want)
    if bad:
        _dump_failure(f"edge_chimeric_{name}", chim, bad, r0, r1)
    assert not bad, f"align: {len(bad)} pairs differ from the reference, first {bad[:3]}"
    cpu = _restatement(name, False)
    bad = _bitwise(inter, cpu, FIELDS)
    assert len(bad) == 0, f"{len(bad)} pairs differ from the restatement, e.g. {inter[bad[0]]} vs {cpu[bad[0]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PAIRED_EDGE_SETS))
def test_gpu_paired_edges_routing(gpu_runs, name):
    """Routing asserted, not only dumped on failure: `writtenBy` (1: pass 1 <128>, 2: pass 1b <256>, 3: pass
    2 <512>, 4: pass 3 on the reference's pools) against the rules the code gives (paired.hip: the host's
    lists by max(L0, L1), align_pair's checks in their order).  Default pools, no env hook.

    A pair with a mate under 50 bases is written by the first pass that sees it, before any length or
    IUPAC check (align_pair's first line, as the reference returns first): pass 1 when the other mate has
    at most 128 bases, else pass 1b, whose list the host put it on -- so the rules for longer pairs hold
    for pairs with both mates of at least 50 bases, and a short-mate pair has its pass asserted exactly.
    A pair with both mates under 50 is cleared by snapgpu_paired_align_batch: writtenBy 0."""
    _, r0, r1, _ = _world(name)
    inter, chim = gpu_runs(name)
    l0, l1 = r0.lengths().astype(int), r1.lengths().astype(int)
    mx, mn = np.maximum(l0, l1), np.minimum(l0, l1)
    for tag, got in (("intersect", inter), ("align", chim)):
        wb, deferred = got["writtenBy"].astype(int), (got["flags"] & snapgpu.PFLAG_DEFERRED) != 0
        both_short = mx < 50
        if tag == "align":
            assert (wb[both_short] == 0).all(), tag
        rest = ~both_short if tag == "align" else np.ones(len(wb), dtype=bool)
        assert ((wb[rest] >= 1) & (wb[rest] <= 4)).all(), tag
        assert (deferred[rest] == (wb[rest] > 1)).all(), tag      # PFLAG_DEFERRED iff a later pass wrote it
        short = (mn < 50) & rest
        assert (wb[short] == np.where(mx[short] <= 128, 1, 2)).all(), tag
        full = mn >= 50
        assert (wb[full & (mx > 256)] >= 3).all(), tag            # 3 or 4
        assert (wb[full & (mx >= 129) & (mx <= 256)] >= 2).all(), tag
        if PAIRED_EDGE_SETS[name][0] == "small.fa":               # the genome with IUPAC bytes
            other = np.array([_has_other(r0, i) or _has_other(r1, i) for i in range(r0.n)])
            sel = other & full & (mx <= 256)
            if name.startswith("long"):
                assert sel.sum() >= 5
            assert (wb[sel] >= 3).all(), tag                      # byte compares: the <512> passes
    if name.startswith("long"):
        wb = inter["writtenBy"].astype(int)
        assert set(wb) >= {1, 2, 3}                               # every length class is routed somewhere else


# The pass-1 / pass-2 pool size (SNAPGPU_PAIRED_POOL1) for the pass-3 assertion: a pair leaves a pass for the
# next when a set pair collects POOL1 / 2 mates (or POOL1 candidates or anchors), the very condition under
# which the restatement flags exhaustion at maxCandidatePoolSize = POOL1.  On the CPU that count is 0 of the
# 120 repeat pairs at 1806 and above, 30 at 1805 and 1804, 63 at 1800, 80 at 1700: 1805 is the largest value
# that sends at least 10 pairs to pass 3.
PASS3_POOL1 = 1805


@pytest.mark.gpu
def test_gpu_repeat_pairs_reach_pass3(gpu_available, gpu_runs, monkeypatch):
    """Pass 3 (paired_kernel<512> on pools of the reference's size) entered by a real overflow of the
    pass-1 / pass-2 pools, not through SNAPGPU_PAIRED_POOL1=2 on ordinary pairs: some repeat pair must
    have writtenBy == 4, with records equal to the restatement's.

    With the default pools (4,096 candidates, 2,048 mates per set pair) no repeat pair leaves pass 1: all
    120 records come back with writtenBy 1 (MI355X), since a set pair collects at most 903 mates, one per
    element copy of one orientation.  So this one assertion runs with SNAPGPU_PAIRED_POOL1 = PASS3_POOL1, the
    largest pool that still overflows for at least 10 pairs: 30 pairs then overflow in pass 1, again in
    pass 1b and pass 2 (the same pools) and are written by pass 3; the other 90 by pass 1."""
    _, r0, r1, _ = _world("repeat_default")
    inter, _ = gpu_runs("repeat_default")
    print("repeat_default, default pools: writtenBy counts",
          dict(zip(*(x.tolist() for x in np.unique(inter["writtenBy"], return_counts=True)))))
    monkeypatch.setenv("SNAPGPU_PAIRED_POOL1", str(PASS3_POOL1))
    pa = _aligner("repeat_default")
    monkeypatch.delenv("SNAPGPU_PAIRED_POOL1")
    got = pa.intersect(r0, r1)
    _no_corrupt_reads(got)
    print(f"repeat_default, SNAPGPU_PAIRED_POOL1={PASS3_POOL1}: writtenBy counts",
          dict(zip(*(x.tolist() for x in np.unique(got["writtenBy"], return_counts=True)))))
    assert int((got["writtenBy"] == 4).sum()) >= 10
    # the pairs that overflow are the ones the restatement cannot complete in a pool of that size
    idx, _, _, p = _world("repeat_default")
    small = oracle_paired(idx, r0, r1, _params(p, maxCandidatePoolSize=PASS3_POOL1), chimeric=False)
    assert np.array_equal(got["writtenBy"] == 4, (small["flags"] & snapgpu.PFLAG_POOL_EXHAUSTED) != 0)
    assert ((got["flags"] & snapgpu.PFLAG_DEFERRED) != 0).sum() == (got["writtenBy"] == 4).sum()
    cpu = _restatement("repeat_default", False)
    bad = _bitwise(got, cpu, FIELDS)
    if len(bad):
        _dump_failure("edge_pass3", got, _cmp(paired_tsv_rows(got, chimeric=False), _want("repeat_default")[0]), r0, r1)
    assert len(bad) == 0, f"{len(bad)} pairs differ from the restatement, e.g. pair {bad[0]}"
    assert not _cmp(paired_tsv_rows(got, chimeric=False), _want("repeat_default")[0])


@pytest.mark.gpu
def test_gpu_long_pairs_independent_of_wave_history(gpu_available, gpu_runs, monkeypatch):
    """`long` on one wave per pass (SNAPGPU_PAIRED_GRID=1) equals the full-grid run bitwise: one wave then
    aligns a 500-base pair, a 50-base one and an IUPAC one in a row, so what PLds<512> and a deferred pair
    leave in LDS and in the pools is covered (test_paired.py's history test never enters <512> with a
    read over 150 bases)."""
    for name in ("long_default", "long_wide"):
        _, r0, r1, _ = _world(name)
        full, _ = gpu_runs(name)
        monkeypatch.setenv("SNAPGPU_PAIRED_GRID", "1")
        pa = _aligner(name)
        monkeypatch.delenv("SNAPGPU_PAIRED_GRID")
        assert max(v for k, v in pa.debug_grids().items() if k.startswith("grid")) == 1
        few = pa.intersect(r0, r1)
        _no_corrupt_reads(few)
        bad = _bitwise(few, full, FIELDS + ("flags", "writtenBy"))
        if len(bad):
            _dump_failure(f"edge_history_{name}", few, _cmp(paired_tsv_rows(few, chimeric=False), _want(name)[0]), r0, r1)
        assert len(bad) == 0, f"{name}: {len(bad)} pairs differ on one wave, e.g. pair {bad[0]}"
    wb = full["writtenBy"].astype(int)
    assert (wb == 3).sum() >= 100 and (wb == 1).sum() >= 10   # the wave's <512> pass took the long and the IUPAC pairs


@pytest.mark.gpu
def test_gpu_pool_exhaustion_flags_and_recovery(gpu_available):
    """SNAPGPU_PFLAG_POOL_EXHAUSTED, named by no test before: with maxCandidatePoolSize EXHAUST_POOL the
    kernel raises it for exactly the repeat pairs the restatement flags (the three sites of paired.hip
    against snap_oracle.c's three), every other pair's record equals the restatement's bitwise, the host
    turns it into SNAPGPU_EINVAL / SnapGpuError("... candidate pool exhausted ..."), and the aligner stays
    usable: the first 200 pairs of paired_{1,2}.fq come out as from a fresh aligner."""
    _, r0, r1, _ = _world("repeat_default")
    cpu = _exhausted_restatement()
    pa = _aligner("repeat_default", maxCandidatePoolSize=EXHAUST_POOL)
    with pytest.raises(snapgpu.SnapGpuError, match="candidate pool exhausted"):
        pa.intersect(r0, r1)
    out = np.zeros(r0.n, dtype=snapgpu.PAIR_RESULT_DTYPE)
    rc = snapgpu.lib().snapgpu_paired_intersect_batch(pa._h, r0._p, r1._p, out.ctypes.data)
    assert rc == SNAPGPU_EINVAL and "candidate pool exhausted" in snapgpu.last_error()
    _no_corrupt_reads(out)
    flagged = (out["flags"] & snapgpu.PFLAG_POOL_EXHAUSTED) != 0
    want = (cpu["flags"] & snapgpu.PFLAG_POOL_EXHAUSTED) != 0
    assert 10 <= int(want.sum()) < len(want)
    assert np.array_equal(flagged, want), (np.nonzero(flagged != want)[0][:10], int(flagged.sum()), int(want.sum()))
    bad = _bitwise(out[~flagged], cpu[~flagged], FIELDS)
    assert len(bad) == 0, f"{len(bad)} unflagged pairs differ from the restatement"
    # the same aligner afterwards: the pairs it completed, as a batch of their own, succeed ...
    keep = np.nonzero(~flagged)[0]
    k0, k1 = (snapgpu.Reads.from_list([r.get(int(i)) for i in keep]) for r in (r0, r1))
    again = pa.intersect(k0, k1)
    assert not (again["flags"] & snapgpu.PFLAG_POOL_EXHAUSTED).any()
    assert len(_bitwise(again, cpu[keep], FIELDS)) == 0
    # ... and the first 200 pairs of paired_{1,2}.fq come out as from a fresh aligner (same index and pools)
    s0, s1 = (snapgpu.Reads.from_fastq(os.path.join(G, f"paired_{k}.fq")).slice(0, 200) for k in (1, 2))
    same = pa.align(s0, s1)
    fresh = _aligner("repeat_default", maxCandidatePoolSize=EXHAUST_POOL).align(s0, s1)
    _no_corrupt_reads(same)
    assert len(_bitwise(same, fresh, FIELDS + ("fromAlignTogether", "alignedAsPair", "nSingleScored", "flags",
                                               "writtenBy"))) == 0
