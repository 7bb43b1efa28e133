"""Forced mode of align_kernel<128> retires the elements its lane prefilter settles (one pending
candidate whose distances fail) without fetching them: they are only counted into nLocationsScored,
each with the score limit in force at its turn (align_score.h forced_filter / score_batched).

The genome is small and repeat-rich, so most reads end in forced mode with many linked elements
(the instrumented oracle counts, for WORLD's 20,000 reads, 7,134 reads with >= 64 of them, 1.61M
settled elements among 1.83M forced pops, and 315 limit changes inside forced mode).  Every record
field stays bit-exact against the oracle, nLocationsScored and both probabilities included.
"""
import numpy as np
import pytest

import snapgpu
from oracle_ffi import mismatches, oracle_align, oracle_align_ex

pytestmark = pytest.mark.gpu

GENOME = dict(total_bases=2_000_000, seed=5, n_contigs=2, n_repeat_families=12, repeat_fraction=0.7)
N_READS = 20_000


@pytest.fixture(scope="module")
def world():
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.synthetic(**GENOME), 20, 8)   # takes ownership of the genome
    reads = snapgpu.Reads.synthetic(snapgpu.Genome.synthetic(**GENOME), N_READS, seed=99)
    return {"index": idx, "reads": reads, "oracle": oracle_align(idx, reads, snapgpu.default_params())}


def _diff(gpu, cpu, bad, k=3):
    return "\n".join(f"read {i}\n  gpu={gpu[i]}\n  cpu={cpu[i]}" for i in bad[:k])


def test_settled_elements_counted_in_order(gpu_available, world):
    """Both paths run and the records equal the oracle's: elements retired without a fetch, and batches
    in which a success lowered the limit ahead of settled positions of their span.
    Observed on MI355X: nForcedSettled = 1,603,142 (the instrumented oracle counts 1.61M), nForcedLimitSpans = 47
    (a subset of the oracle's 315 limit changes: those with a settled position after them in their batch's span)."""
    al = snapgpu.BaseAligner(world["index"])
    gpu = al.AlignReads(world["reads"])
    t = al.timing()
    print(f"nForcedSettled={t['nForcedSettled']} nForcedLimitSpans={t['nForcedLimitSpans']}")
    bad = mismatches(gpu, world["oracle"])
    assert len(bad) == 0, f"{len(bad)} of {len(gpu)} differ\n" + _diff(gpu, world["oracle"], bad)
    assert t["nForcedSettled"] > 0
    assert t["nForcedLimitSpans"] > 0


# limits that stay in the pair filter's range; limits that start above the filter's 7 and fall into quad and
# pair range while forced mode runs
PARAM_SETS = [dict(maxK=5, extraSearchDepth=1), dict(maxK=8, extraSearchDepth=1), dict(maxK=8, extraSearchDepth=5)]


@pytest.mark.parametrize("kw", PARAM_SETS, ids=[",".join(f"{k}={v}" for k, v in p.items()) for p in PARAM_SETS])
def test_limits_across_filter_boundaries(gpu_available, world, kw):
    reads = world["reads"].slice(0, 5000)
    al = snapgpu.BaseAligner(world["index"], **kw)
    gpu = al.AlignReads(reads)
    cpu = oracle_align(world["index"], reads, al.params)
    bad = mismatches(gpu, cpu)
    assert len(bad) == 0, f"{kw}: {len(bad)} of {len(gpu)} differ\n" + _diff(gpu, cpu, bad)
    assert al.timing()["nForcedSettled"] > 0


def test_multihit_twin(gpu_available, world):
    """align_kernel<128, true> (multi-hit export, 8 hits per read) takes the same paths."""
    reads = world["reads"].slice(0, 5000)
    al = snapgpu.BaseAligner(world["index"])
    res, found, hits = al.AlignReadsEx(reads, None, 8)
    wres, wfound, whits = oracle_align_ex(world["index"], reads, al.params, None, 8)
    bad = mismatches(res, wres)
    assert len(bad) == 0, f"{len(bad)} of {len(res)} differ\n" + _diff(res, wres, bad)
    assert np.array_equal(found, wfound)
    for i in np.nonzero(wfound > 0)[0]:
        assert np.array_equal(hits[i, :wfound[i]], whits[i, :wfound[i]]), i
    assert al.timing()["nForcedSettled"] > 0


def test_stream_equals_resident(gpu_available, world):
    al = snapgpu.BaseAligner(world["index"])
    stream = al.AlignReads(world["reads"])
    ts = al.timing()
    dev = al.upload(world["reads"])
    dev.run()
    resident = dev.results()
    tr = al.timing()
    assert np.array_equal(stream.view(np.uint8), resident.view(np.uint8))
    assert (ts["nForcedSettled"], ts["nForcedLimitSpans"]) == (tr["nForcedSettled"], tr["nForcedLimitSpans"])
