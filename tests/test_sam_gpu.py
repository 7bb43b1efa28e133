"""SAM text formatted on the GPU (csrc/sam_format.hip: length pass, scan, LDS-staged write pass):
byte-identical to the host formatter and, through it, to the reference writer's own lines
(tests/golden/expected_small.sam.gz, expected_small_clipped.sam.gz)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import snapgpu
from bam_cases import made_up
from oracle_ffi import oracle_align, oracle_cigars
from sam_cases import (G, READ_GROUPS, cigars_from_pairs, clipped_case, fabricated_case, fastq, small_case,
                       small_index)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def idx():
    return small_index()


@pytest.fixture(scope="module")
def aligner(gpu_available, idx):
    return snapgpu.BaseAligner(idx)


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    """small_world's reads with ids, oracle records and CIGARs, the host formatter's text of every
    line, and one aligner: computed once, shared by the tests below, never modified."""
    idx, reads = small_world["index"], small_world["reads"]
    res = oracle_align(idx, reads, snapgpu.default_params())
    loc, dirs = snapgpu.cigar_inputs(res)
    cig = cigars_from_pairs(oracle_cigars(idx, [reads.get(i)[0] for i in range(reads.n)], loc, dirs, 0))
    ids = [b"read_%d extra" % i for i in range(reads.n)]
    lines = snapgpu.sam_format(idx, reads, ids, res, cig).splitlines(keepends=True)
    assert len(lines) == reads.n
    return dict(idx=idx, genome=small_world["genome"], reads=reads, res=res, cig=cig, ids=ids, lines=lines, aligner=snapgpu.BaseAligner(idx))


def _expected(name, use_m):
    return gzip.open(os.path.join(G, name), "rt").read().splitlines()[use_m::2]


def _same_lines(got, want):
    got = got.decode().splitlines()
    bad = [(a, b) for a, b in zip(got, want) if a != b]
    assert len(got) == len(want) and not bad, f"{len(bad)} differ: {bad[:2]}"


def _resident(aligner, reads, use_m, ids=None):
    dev = aligner.upload(reads)
    dev.run()
    dev.run_cigars(useM=use_m)
    dev.run_sam(reads, ids=ids)
    return dev.sam()


# --------------------------------------------------------------- reference pins
@pytest.mark.parametrize("use_m", [0, 1])
def test_resident_sam_matches_reference(aligner, use_m):
    """upload -> run -> run_cigars -> run_sam -> sam() on small_reads.fq (the batch's own ids)."""
    reads = snapgpu.Reads.from_fastq(os.path.join(G, "small_reads.fq"))
    _same_lines(_resident(aligner, reads, use_m), _expected("expected_small.sam.gz", use_m))


@pytest.mark.parametrize("use_m", [0, 1])
def test_resident_clipped_sam_matches_reference(aligner, use_m):
    """The clipped batch (reads.clip(3)): soft clips, unclipped SEQ / QUAL from the resident reads."""
    reads = snapgpu.Reads.from_fastq(os.path.join(G, "small_reads.fq"))
    reads.clip(3)
    ids = [i for i, _, _ in fastq(os.path.join(G, "small_reads.fq"))]
    _same_lines(_resident(aligner, reads, use_m, ids=ids), _expected("expected_small_clipped.sam.gz", use_m))


def test_resident_back_clip_past_the_upload(aligner, idx, tmp_path):
    """A batch whose last read is clipped at the back: snapgpu_reads_upload copies bases and qualities
    up to the largest clipped end, so the clipped bytes SEQ / QUAL print are not resident; run_sam
    uploads them.  The first 580 small reads (read 579 is back-clipped), twice on one resident batch."""
    fq = fastq(os.path.join(G, "small_reads.fq"))[:580]
    path = tmp_path / "head.fq"
    path.write_text("".join(f"@{i}\n{b}\n+\n{q}\n" for i, b, q in fq))
    reads = snapgpu.Reads.from_fastq(str(path))
    front, full = reads.clip(3)
    assert int(full[-1]) > int(front[-1]) + int(reads.lengths()[-1])   # the last read is clipped at the back
    dev = aligner.upload(reads)
    dev.run()
    dev.run_cigars()
    want = snapgpu.sam_format(idx, reads, [i for i, _, _ in fq], dev.results(), dev.cigars(), clip=(front, full))
    assert want.splitlines()[-1].decode() == _expected("expected_small_clipped.sam.gz", 0)[579]
    for _ in range(2):
        dev.run_sam(reads)          # the batch's own ids
        assert dev.sam() == want


@pytest.mark.parametrize("use_m", [0, 1])
def test_batch_sam_matches_reference(aligner, idx, use_m):
    """BaseAligner.sam_format over the reference's own records and oracle CIGARs."""
    reads, ids, res, cig, _ = small_case(idx, use_m)
    _same_lines(aligner.sam_format(reads, ids, res, cig), _expected("expected_small.sam.gz", use_m))
    reads, ids, res, cig, clip = clipped_case(idx, use_m)
    _same_lines(aligner.sam_format(reads, ids, res, cig, clip=clip), _expected("expected_small_clipped.sam.gz", use_m))


# ----------------------------------------------------------------- differential
@pytest.mark.parametrize("read_group", READ_GROUPS)
def test_fabricated_records_match_host_formatter(aligner, idx, read_group):
    reads, ids, res, cig, _ = fabricated_case(idx)
    want = snapgpu.sam_format(idx, reads, ids, res, cig, read_group=read_group)
    got = aligner.sam_format(reads, ids, res, cig, read_group=read_group)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        pytest.fail(f"{len(got)} vs {len(want)} bytes, {len(bad)} lines differ, first {bad[:3]}: "
                    f"{g[bad[0]][:200] if bad else b''!r} vs {w[bad[0]][:200] if bad else b''!r}")


def _batch_sizes():
    r, t = snapgpu.SAM_RECORDS_PER_WORKGROUP, snapgpu.SAM_SCAN_TILE
    return sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, r - 1, r, r + 1, t - 1, t, t + 1})


def _slice(world, n, start=0):
    """The first n reads (from `start`) as their own batch, with their inputs and the host's text."""
    c = snapgpu.Cigars(world["cig"].editDistance[start:start + n], world["cig"].nOps[start:start + n],
                       world["cig"].ops[start:start + n])
    return (world["reads"].slice(start, n), world["ids"][start:start + n], world["res"][start:start + n], c,
            b"".join(world["lines"][start:start + n]))


@pytest.mark.parametrize("n", _batch_sizes())
def test_batch_sizes(world, n):
    """Around the wave, the workgroup's records (SAM_RECORDS_PER_WORKGROUP) and the scan tile."""
    reads, ids, res, cig, want = _slice(world, n)
    assert world["aligner"].sam_format(reads, ids, res, cig) == want


def test_records_that_pass_the_lds_window(aligner, idx):
    """40 reads of 500 bases with 200-byte ids: a workgroup's 32 lines are some 40 KB of text, composed
    in several 16 KiB windows, unsorted and sorted (mapped in descending order, both directions, some
    unmapped; 1, 3 and 64 CIGAR ops)."""
    n = 40
    v = idx.view()
    piece1 = int(C.cast(v.pieceOffsets, C.POINTER(C.c_uint32))[1])
    locs = [0xFFFFFFFF if i % 9 == 4 else piece1 + 50 + 3 * (n - i) for i in range(n)]
    ids = [b"%03d" % i + b"w" * 197 for i in range(n)]
    reads, ids, res, cig = made_up(locs, [500] * n, [i % 7 for i in range(n)], directions=[i & 1 for i in range(n)],
                                   ids=ids, n_ops=[(1, 3, 64)[i % 3] for i in range(n)])
    want = snapgpu.sam_format(idx, reads, ids, res, cig)
    lines = want.splitlines(keepends=True)
    assert len(lines) == n and all(len(l.split(b"\t")[0]) == 200 and len(l.split(b"\t")[9]) == 500 for l in lines)
    assert sum(len(l) for l in lines[:snapgpu.SAM_RECORDS_PER_WORKGROUP]) > 2 * 16384
    assert aligner.sam_format(reads, ids, res, cig) == want
    text, order = aligner.sam_format(reads, ids, res, cig, sorted_output=True, return_order=True)
    assert np.array_equal(order, np.argsort(snapgpu.sam_sort_keys(idx, res), kind="stable"))
    assert not np.array_equal(order, np.arange(n))
    assert sum(len(lines[int(i)]) for i in order[:snapgpu.SAM_RECORDS_PER_WORKGROUP]) > 2 * 16384
    assert text == b"".join(lines[int(i)] for i in order) == snapgpu.sam_sort_records(idx, want)


def test_buffer_reuse_growing_then_shrinking(world):
    """One aligner's grow-only buffers across calls of growing, then shrinking n and shifted slices."""
    for start, n in ((0, 5), (7, 300), (100, 3900), (3999, 1), (0, 4000), (50, 64), (0, 0), (1234, 33)):
        reads, ids, res, cig, want = _slice(world, n, start)
        assert world["aligner"].sam_format(reads, ids, res, cig) == want, (start, n)


def test_resident_sam_ordered_before_next_run(world):
    """run(); run_cigars(); run_sam(); run(); sam() on one resident batch: the SAM kernels read the
    records on the side stream, the second run's pre-fill and passes rewrite them on the lanes and
    must wait -- the text equals a clean sequence's, repeated 3 times."""
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    clean = al.upload(reads)
    clean.run()
    clean.run_cigars()
    clean.run_sam(reads, ids=ids)
    want = clean.sam()
    assert want == snapgpu.sam_format(world["idx"], reads, ids, clean.results(), clean.cigars())
    dev = al.upload(reads)
    for _ in range(3):
        dev.run()
        dev.run_cigars()
        dev.run_sam(reads, ids=ids)
        dev.run()
        assert dev.sam() == want
    k, d = al.sam_ms()
    assert k > 0 and d > 0


# ------------------------------------------------------------------------ errors
def test_errors_raise_without_device_faults(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = al.upload(reads)
    dev.run()
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_cigar_resident before"):
        dev.run_sam(reads, ids=ids)
    dev.run_cigars()
    with pytest.raises(snapgpu.SnapGpuError, match="does not match the resident batch"):
        dev.run_sam(reads.slice(0, reads.n - 1), ids=ids[:-1])
    with pytest.raises(snapgpu.SnapGpuError, match="does not match the resident batch"):
        dev.run_sam(snapgpu.Reads.synthetic(world["genome"], reads.n, seed=5, read_length=99), ids=ids)
    with pytest.raises(snapgpu.SnapGpuError, match="no read ids"):
        dev.run_sam(reads)          # a synthetic batch carries no ids
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_sam_resident before"):
        dev.sam()
    # cap too small: non-zero, `used` set to the needed size
    dev.run_sam(reads, ids=ids)
    used = C.c_uint64()
    buf = C.create_string_buffer(16)
    rc = snapgpu.lib().snapgpu_sam_download(al._h, dev._h, buf, 16, C.byref(used))
    want = dev.sam()
    assert rc != 0 and used.value == len(want) and "too small" in snapgpu.last_error()
    assert want == snapgpu.sam_format(world["idx"], reads, ids, dev.results(), dev.cigars())
    # an unclipped read longer than 1024 (the host formatter's limit)
    long_reads = snapgpu.Reads.from_list([("A" * 1025, "I" * 1025)])
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        al.sam_format(long_reads, ["r"], np.zeros(1, dtype=snapgpu.RESULT_DTYPE), snapgpu.Cigars.empty(1))
    bad = snapgpu.Cigars.empty(1)
    bad.nOps[0] = 65
    with pytest.raises(snapgpu.SnapGpuError, match="nOps"):
        al.sam_format(snapgpu.Reads.from_list([("ACGT", "IIII")]), ["r"], np.zeros(1, dtype=snapgpu.RESULT_DTYPE), bad)
    # the aligner still works
    reads1, ids1, res1, cig1, want1 = _slice(world, 10)
    assert al.sam_format(reads1, ids1, res1, cig1) == want1
