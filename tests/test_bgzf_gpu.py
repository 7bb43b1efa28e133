"""BGZF members compressed on the GPU (csrc/bgzf.hip: compress pass, scan, gather pass, check): byte-identical
to the host model (snapgpu.bgzf_compress_model), which test_bgzf_model.py holds to the format and to zlib's
inflater.  Every expected value here comes from the model or from gzip."""
import ctypes as C
import gzip

import numpy as np
import pytest

import snapgpu
from bgzf_cases import BLOCK, EOF_BLOCK, SIZED, SIZES, special

pytestmark = pytest.mark.gpu

MAX_INPUT = 4 * BLOCK     # the golden records are cut to four blocks


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    """small_world's 4,000 reads with ids, aligned once on the device, and one aligner; never modified."""
    idx, reads = small_world["index"], small_world["reads"]
    al = snapgpu.BaseAligner(idx)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    ids = [b"read_%d extra" % i for i in range(reads.n)]
    return dict(idx=idx, reads=reads, ids=ids, aligner=al, dev=dev, res=dev.results(), cig=dev.cigars())


def _same(got, want):
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{len(got)} vs {len(want)} bytes, first difference at byte {first} (block {None if first is None else first // BLOCK})")


def _cases():
    return [(c, n) for c in sorted(SIZED) for n in SIZES] + [(name, None) for name in sorted(special())]


@pytest.mark.parametrize("content,n", _cases())
def test_batch_form_matches_the_model(world, content, n):
    data = SIZED[content](n) if n is not None else special()[content][:MAX_INPUT]
    want = snapgpu.bgzf_compress_model(data)
    _same(world["aligner"].bgzf_compress(data), want)
    if n in (BLOCK + 1, None):
        _same(world["aligner"].bgzf_compress(data, eof=False), want[:-28])
        _same(world["aligner"].bgzf_compress(data), want)      # the same bytes again


@pytest.mark.parametrize("sorted_output", [False, True])
def test_resident_chain(world, sorted_output):
    dev, reads, ids = world["dev"], world["reads"], world["ids"]
    dev.run_bam(reads, ids=ids, sorted_output=sorted_output)
    dev.run_bgzf()
    out = dev.bgzf()
    raw = dev.bam()                                # still the records, after the compression
    assert len(raw) > 10 * BLOCK
    _same(out, snapgpu.bgzf_compress_model(raw))
    assert gzip.decompress(out) == raw
    want, _ = snapgpu.bam_format(world["idx"], reads, ids, world["res"], world["cig"])
    assert (raw == want) != sorted_output and len(raw) == len(want)
    _same(dev.bgzf(eof=False) + EOF_BLOCK, out)


def _slice(world, n, start=0):
    c = snapgpu.Cigars(world["cig"].editDistance[start:start + n], world["cig"].nOps[start:start + n],
                       world["cig"].ops[start:start + n])
    return world["reads"].slice(start, n), world["ids"][start:start + n], world["res"][start:start + n], c


def test_buffer_reuse_growing_then_shrinking(world):
    al = world["aligner"]
    for start, n in ((0, 5), (7, 300), (0, 4000), (3999, 1), (0, 0), (1234, 33)):
        reads, ids, res, cig = _slice(world, n, start)
        if n == 0:                                 # no records: the batch forms, on the same aligner
            raw = al.bam_format(reads, ids, res, cig)[0]
            out = al.bgzf_compress(raw)
        else:
            dev = al.upload(reads)
            dev.run()
            dev.run_cigars()
            dev.run_bam(reads, ids=ids)
            dev.run_bgzf()
            out, raw = dev.bgzf(), dev.bam()
        _same(out, snapgpu.bgzf_compress_model(raw))
        assert (out == EOF_BLOCK) == (n == 0)
    raw = snapgpu.bam_format(world["idx"], *_slice(world, 2000))[0]
    for size in (2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, BLOCK, 0, 3 * BLOCK + 1):
        assert len(raw) >= size
        _same(al.bgzf_compress(raw[:size]), snapgpu.bgzf_compress_model(raw[:size]))


def test_ordered_before_the_next_run(world):
    """run_bam; run_bgzf; run; run_cigars; bgzf() three times on one resident batch: the compressor reads the
    records on the stream that wrote them, whatever the lanes do meanwhile."""
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    dev.run_bam(reads, ids=ids)
    want = snapgpu.bgzf_compress_model(dev.bam())
    for _ in range(3):
        dev.run_bam(reads, ids=ids)
        dev.run_bgzf()
        dev.run()
        dev.run_cigars()
        _same(dev.bgzf(), want)
    k, d = al.bgzf_ms()
    assert k > 0 and d > 0


def test_errors_raise_and_the_aligner_still_works(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_bam_resident before"):
        dev.run_bgzf()
    dev.run_bam(reads, ids=ids)
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_bam_bgzf_resident since"):
        dev.bgzf()
    dev.run_bgzf()
    want = snapgpu.bgzf_compress_model(dev.bam())
    _same(dev.bgzf(), want)
    dev.run_bam(reads, ids=ids)                    # the records are written again: the stream is stale
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_bam_bgzf_resident since"):
        dev.bgzf()
    dev.run_bgzf()
    used = C.c_uint64()
    buf = C.create_string_buffer(16)
    rc = snapgpu.lib().snapgpu_bam_bgzf_download(al._h, dev._h, 1, buf, 16, C.byref(used))
    assert rc != 0 and used.value == len(want) and "too small" in snapgpu.last_error()
    _same(dev.bgzf(), want)
    data = special()["fibonacci"]
    rc = snapgpu.lib().snapgpu_bgzf_compress_gpu(al._h, data, len(data), 1, buf, 16, C.byref(used))
    assert rc != 0 and used.value == len(snapgpu.bgzf_compress_model(data)) and "too small" in snapgpu.last_error()
    assert snapgpu.lib().snapgpu_bgzf_compress_gpu(al._h, None, 5, 1, buf, 16, C.byref(used)) != 0
    _same(al.bgzf_compress(data), snapgpu.bgzf_compress_model(data))
    _same(al.bgzf_compress(b""), EOF_BLOCK)
    assert al.bgzf_compress(b"", eof=False) == b""
