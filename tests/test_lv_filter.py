"""The forced-mode prefilter of align_kernel<128>, unit-tested on the device: lv_filter_kernel
(snapgpu.lv_filter_batch) does, from a task's (read, loc, dir, s, k) upward, what forced_filter does --
substring_ok, the lane's masks from the aligner's genome planes (the very statements forced_filter runs),
lv_pair_dist / lv_quad_dist forward, the ballot, the reverse call at k - e1, the result encoding -- with 32 tasks
per wave in the lane-pair form and 16 in the lane-quad form.  tests/c/lv_lane_test.cpp checks a host restatement
of the pair and quad arithmetic; this checks the device functions themselves, their DPP lane exchange and the
funnel-shift mask build, outer diagonals included.  The reference is the oracle's LandauVishkin on the genome's
bytes, called as BaseAligner::score calls it; the encoded words must be equal.

test_filter_tasks_cover (no GPU) checks with the oracle alone that the tasks reach every diagonal."""
import numpy as np
import pytest

import lv_cases
import snapgpu


def _write_fasta(path, contigs):
    with open(path, "w") as f:
        for name, seq in contigs:
            f.write(f">{name}\n")
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
    return str(path)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    fa = _write_fasta(tmp_path_factory.mktemp("lvf") / "two.fa", lv_cases.filter_genome())
    g = snapgpu.Genome.from_fasta(fa, lv_cases.FILTER_PADDING)
    n_bases = g.n_bases
    pieces = [off for _, off in g.pieces]
    assert len(pieces) == 2 and 19_000 < n_bases < 23_000
    bases = g.bases() + b"n" * 256     # the bytes LV may look at past the genome's end (the device copy's guard)
    return dict(fasta=fa, bases=bases, pieces=pieces, n_bases=n_bases, cache={})


def _tasks(world, quad):
    if quad not in world["cache"]:
        T = lv_cases.filter_tasks(quad, world["bases"], world["pieces"], world["n_bases"])
        E = [lv_cases.expected_filter(t, world["bases"], world["pieces"], world["n_bases"]) for t in T]
        world["cache"][quad] = (T, E)
    return world["cache"][quad]


@pytest.mark.parametrize("quad", [False, True], ids=["pair", "quad"])
def test_filter_tasks_cover(world, quad):
    T, E = _tasks(world, quad)
    KM = lv_cases.LQ_K if quad else lv_cases.FKM
    per = 16 if quad else 32
    assert len(T) % per == 1 and len(T) <= 10_000          # the last wave holds a single task
    assert {(t[1] - KM + 1024) & 31 for t in T} == set(range(32))      # every phase of the plane window
    assert any(t[1] < KM for t in T)
    assert {t[4] for t in T} == set(range(KM + 1))
    # a window that ends exactly at the servable range's end (the genome's end + N_PADDING) is settled, one base
    # further it is not; windows over the two contigs' ends are served (they are shorter than the padding)
    nb = world["n_bases"] + lv_cases.NPAD
    ends = {t[1] + len(t[0]) + lv_cases.MAX_K - nb: e[0] != 0 for t, e in zip(T, E) if t[5]}
    assert ends.get(0) is True and ends.get(-1) is True and ends.get(1) is False, ends
    c1 = world["pieces"][1]
    for edge in (c1 - lv_cases.FILTER_PADDING, c1):
        assert {t[1] + len(t[0]) + lv_cases.MAX_K - edge for t in T} >= {-1, 0, 1}
    assert sum(1 for t in T if not t[5]) >= 10
    # every diagonal, both LV directions, both read directions: a pure indel path of |d| steps ending on +-d
    for lvdir, (ei, ni) in (("f", (1, 3)), ("r", (2, 4))):
        for rc in (0, 1):
            for d in [x for a in range(1, KM + 1) for x in (a, -a)]:
                cnt = sum(1 for t, e in zip(T, E) if e[0] and t[2] == rc and e[ei] == abs(d) and e[ni] == d)
                assert cnt >= 8, (lvdir, rc, d, cnt)
    fails = sum(1 for e in E if e[0] and (e[1] < 0 or e[2] < 0))
    assert 4 * fails >= len(T), (fails, len(T))
    assert sum(1 for e in E if e[0] and e[1] >= 0 and e[2] >= 0) >= 200
    # neighbours in a wave differ: active next to inactive, exact match next to failure
    kinds = [0 if not t[5] or not e[0] else 1 if (e[1], e[2]) == (0, 0) else 2 if e[1] < 0 or e[2] < 0 else 3
             for t, e in zip(T, E)]
    pairs = {(a, b) for a, b in zip(kinds, kinds[1:])}
    assert {(0, 1), (1, 2), (2, 1), (2, 3), (0, 2), (3, 0)} <= pairs | {(b, a) for a, b in pairs}, pairs


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    fa = _write_fasta(tmp_path_factory.mktemp("lvm") / "many.fa", lv_cases.filter_genome_many())
    g = snapgpu.Genome.from_fasta(fa, lv_cases.MANY_PADDING)
    pieces = [off for _, off in g.pieces]
    assert len(pieces) > 100
    return dict(fasta=fa, bases=g.bases() + b"n" * 256, pieces=pieces, n_bases=g.n_bases)


def _edge_tasks(many, quad):
    T = lv_cases.filter_edge_tasks(quad, many["bases"], many["pieces"], many["n_bases"])
    return T, [lv_cases.expected_filter(t, many["bases"], many["pieces"], many["n_bases"], lv_cases.MANY_PADDING)
               for t in T]


@pytest.mark.parametrize("quad", [False, True], ids=["pair", "quad"])
def test_filter_edge_tasks_cover(many, quad):
    """Windows at the end of a contig's piece: settled up to the next contig's start, never past it."""
    T, E = _edge_tasks(many, quad)
    for t, e in zip(T, E):
        nxt = min(p for p in many["pieces"] if p > t[1])
        past = t[1] + len(t[0]) + lv_cases.MAX_K - nxt
        assert (e[0] != 0) == (past <= 0), (t[1:], past)
    pasts = {t[1] + len(t[0]) + lv_cases.MAX_K - min(p for p in many["pieces"] if p > t[1]) for t in T}
    assert pasts >= {-1, 0, 1, 2, 3}
    assert sum(1 for e in E if e[0] == 0) >= 40 and sum(1 for e in E if e[0] and e[1] >= 0 and e[2] >= 0) >= 30


@pytest.mark.gpu
@pytest.mark.parametrize("quad", [False, True], ids=["pair", "quad"])
def test_gpu_lv_filter_contig_ends(gpu_available, many, quad):
    T, E = _edge_tasks(many, quad)
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.from_fasta(many["fasta"], lv_cases.MANY_PADDING),
                                    lv_cases.FILTER_SEED_LEN, 4)
    al = snapgpu.BaseAligner(idx, device=0)
    got = snapgpu.lv_filter_batch(al, quad, T)
    want = np.array([e[0] for e in E], dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), *T[i][1:5], hex(got[i]), hex(want[i])) for i in bad[:5]]


@pytest.mark.gpu
@pytest.mark.parametrize("quad", [False, True], ids=["pair", "quad"])
def test_gpu_lv_filter_matches_oracle(gpu_available, world, quad):
    T, E = _tasks(world, quad)
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.from_fasta(world["fasta"], lv_cases.FILTER_PADDING),
                                    lv_cases.FILTER_SEED_LEN, 4)
    al = snapgpu.BaseAligner(idx, device=0)
    got = snapgpu.lv_filter_batch(al, quad, T)     # one launch
    want = np.array([e[0] for e in E], dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"{len(bad)} of {len(T)} tasks differ from the oracle, first (index, loc, dir, s, k, n, "
                           f"got, want): {[(int(i), *T[i][1:5], len(T[i][0]), hex(got[i]), hex(want[i])) for i in bad[:5]]}")
