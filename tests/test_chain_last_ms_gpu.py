"""Lifetime of the output chain's "last call" times (csrc/output_chain.hip: sam_ms, bam_ms, bgzf_ms, bai_ms,
dupmark_ms): nothing before a stage's first device call, the resident batch's state after the chain, nothing
again once that batch is released (the aligner must not point at freed state), a value again after a
batch-form call."""
import gc
import math
import os

import pytest

import snapgpu
from sam_cases import G, fastq, small_index

pytestmark = pytest.mark.gpu

NOTHING = {"sam_ms": "no device SAM call", "bam_ms": "no device BAM call", "bgzf_ms": "no device BGZF call",
           "bai_ms": "no device BAI call", "dupmark_ms": "no device duplicate marking"}


def _all_raise(aligner):
    for name, text in NOTHING.items():
        with pytest.raises(snapgpu.SnapGpuError, match=text):
            getattr(aligner, name)()


def test_last_ms_follows_the_state_it_times(gpu_available):
    fq = fastq(os.path.join(G, "small_reads.fq"))[:64]
    reads = snapgpu.Reads.from_list([(b, q) for _, b, q in fq])
    ids = [i.encode() for i, _, _ in fq]
    aligner = snapgpu.BaseAligner(small_index())
    dev = aligner.upload(reads)
    dev.run()
    dev.run_cigars()
    _all_raise(aligner)                                  # a. no device call of any stage yet
    dev.run_sam(reads, ids=ids)
    dev.run_bam(reads, ids=ids, sorted_output=True)
    dev.run_dupmark()
    dev.run_bgzf()
    dev.run_bai()
    for name in NOTHING:                                 # b. the resident chain's times
        k, d = getattr(aligner, name)()
        assert math.isfinite(k) and math.isfinite(d) and k >= 0 and d >= 0, (name, k, d)
    del dev
    gc.collect()
    _all_raise(aligner)                                  # c. the state they timed is gone
    aligner.bgzf_compress(b"x" * 100)
    k, d = aligner.bgzf_ms()
    assert math.isfinite(k) and math.isfinite(d) and k >= 0 and d >= 0
    for name in sorted(set(NOTHING) - {"bgzf_ms"}):
        with pytest.raises(snapgpu.SnapGpuError, match=NOTHING[name]):
            getattr(aligner, name)()
