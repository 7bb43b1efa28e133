"""BAM records encoded on the GPU (csrc/bam_format.hip: length pass, NM carry scan, size scan,
LDS-staged write pass): byte-identical to the host encoder (snapgpu.bam_format), which
test_bam_host.py pins to the reference writer's own records.  Every expected value here comes from
the host encoder."""
import ctypes as C
import os

import numpy as np
import pytest

import snapgpu
from bam_cases import fields, made_up, permuted, split_records
from sam_cases import G, READ_GROUPS, fabricated_case, fastq, small_index

pytestmark = pytest.mark.gpu

TILE = snapgpu.SAM_SCAN_TILE
GROUP = snapgpu.SAM_RECORDS_PER_WORKGROUP


@pytest.fixture(scope="module")
def idx():
    return small_index()


@pytest.fixture(scope="module")
def aligner(gpu_available, idx):
    return snapgpu.BaseAligner(idx)


@pytest.fixture(scope="module")
def pieces(idx):
    v = idx.view()
    return [int(x) for x in C.cast(v.pieceOffsets, C.POINTER(C.c_uint32))[:v.nPieces]]


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    """small_world's 4,000 reads with ids, aligned once on the device: records, CIGARs, the host
    encoder's record of every read (carry-in 0) and one aligner, shared below and never modified."""
    idx, reads = small_world["index"], small_world["reads"]
    al = snapgpu.BaseAligner(idx)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    res, cig = dev.results(), dev.cigars()
    ids = [b"read_%d extra" % i for i in range(reads.n)]
    raw, carry = snapgpu.bam_format(idx, reads, ids, res, cig)
    recs = split_records(raw)
    assert len(recs) == reads.n
    return dict(idx=idx, genome=small_world["genome"], reads=reads, res=res, cig=cig, ids=ids, raw=raw, recs=recs,
                carry=carry, aligner=al)


@pytest.fixture(scope="module")
def fab(idx):
    """sam_cases.fabricated_case: 5,000 records that reach every branch, built once."""
    return fabricated_case(idx)[:4]


def _key_order(idx, res):
    return np.argsort(snapgpu.bam_sort_keys(idx, res), kind="stable").astype(np.uint32)


def _same(got, want):
    if got != want:
        g, w = split_records(got), split_records(want)
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        pytest.fail(f"{len(got)} vs {len(want)} bytes, {len(g)} vs {len(w)} records, {len(bad)} differ, first "
                    f"#{bad[:1]}: {fields(g[bad[0]]) if bad else ''} vs {fields(w[bad[0]]) if bad else ''}")


# ------------------------------------------------------------------------ parity
@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clip3"])
@pytest.mark.parametrize("use_m", [0, 1])
def test_resident_bam_matches_host_encoder(aligner, idx, use_m, clip):
    """upload -> run -> run_cigars -> run_bam -> bam() on small_reads.fq against the host encoder over
    the downloaded records and CIGARs."""
    reads = snapgpu.Reads.from_fastq(os.path.join(G, "small_reads.fq"))
    c = reads.clip(3) if clip else None
    ids = [i for i, _, _ in fastq(os.path.join(G, "small_reads.fq"))]
    dev = aligner.upload(reads)
    dev.run()
    dev.run_cigars(useM=use_m)
    dev.run_bam(reads, ids=ids if clip else None)     # unclipped: the batch's own ids
    want, carry = snapgpu.bam_format(idx, reads, ids, dev.results(), dev.cigars(), clip=c)
    _same(dev.bam(), want)
    assert dev.bam_nm_carry() == carry
    assert len(split_records(want)) == reads.n


@pytest.mark.parametrize("read_group", READ_GROUPS)
def test_fabricated_records_match_host_encoder(aligner, idx, fab, read_group):
    reads, ids, res, cig = fab
    want, carry = snapgpu.bam_format(idx, reads, ids, res, cig, read_group=read_group, nm_carry=2)
    got, got_carry = aligner.bam_format(reads, ids, res, cig, read_group=read_group, nm_carry=2)
    _same(got, want)
    assert got_carry == carry


# ------------------------------------------------------- shapes where the kernel can go wrong
def _slice(world, n, start=0):
    c = snapgpu.Cigars(world["cig"].editDistance[start:start + n], world["cig"].nOps[start:start + n],
                       world["cig"].ops[start:start + n])
    return world["reads"].slice(start, n), world["ids"][start:start + n], world["res"][start:start + n], c


def _batch_sizes():
    return sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, GROUP - 1, GROUP, GROUP + 1, TILE - 1, TILE, TILE + 1})


@pytest.mark.parametrize("n", _batch_sizes())
def test_batch_sizes(world, n):
    """Around the wave, the workgroup's records and the scan tile (of both scans)."""
    reads, ids, res, cig = _slice(world, n)
    want, carry = snapgpu.bam_format(world["idx"], reads, ids, res, cig, nm_carry=9)
    got, got_carry = world["aligner"].bam_format(reads, ids, res, cig, nm_carry=9)
    _same(got, want)
    assert got_carry == carry


@pytest.mark.parametrize("read_group", [None, "FASTQ"])
def test_read_lengths_parities_and_directions(aligner, idx, pieces, read_group):
    """Lengths 1, 2, 63, 64, 65, 127 and 1024 (both nibble parities, one and several lane strides),
    forward and RC, mapped and unmapped, with ids of 1 and 254 bytes."""
    lengths = [1, 2, 63, 64, 65, 127, 1024] * 3
    dirs = [0] * 7 + [1] * 7 + [1] * 7
    locs = [pieces[1] + 50 + 3 * i for i in range(14)] + [0xFFFFFFFF] * 7
    ids = [(b"i", b"j" * 254)[i % 2] for i in range(21)]
    reads, ids, res, cig = made_up(locs, lengths, list(range(21)), directions=dirs, ids=ids)
    want, _ = snapgpu.bam_format(idx, reads, ids, res, cig, read_group=read_group)
    f = [fields(r) for r in split_records(want)]
    assert [x["lseq"] for x in f] == lengths and [x["flag"] & 0x10 for x in f] == [0] * 7 + [16] * 7 + [0] * 7
    _same(aligner.bam_format(reads, ids, res, cig, read_group=read_group)[0], want)


def test_no_ops_and_sixty_six_ops(aligner, idx, pieces):
    """nOps 0 (a mapped record whose only ops are its clips, and one without any), and nOps 64 between
    a front and a back soft clip: 66 ops, forward and RC."""
    quals = "##" + "I" * 70 + "###"
    reads = snapgpu.Reads.from_list([("ACGT" * 18 + "ACG", quals)] * 6)
    clip = reads.clip(3)
    assert clip[0].tolist() == [2] * 6 and reads.lengths().tolist() == [70] * 6
    res = np.zeros(6, dtype=snapgpu.RESULT_DTYPE)
    res["result"], res["mapq"] = snapgpu.SingleHit, 40
    res["location"] = [pieces[0] + 10 * (i + 1) for i in range(6)]
    res["direction"] = [0, 1, 0, 1, 0, 1]
    cig = snapgpu.Cigars.empty(6)
    cig.editDistance[:] = [4, 5, 0, 1, -1, 2]
    cig.nOps[:] = [64, 64, 0, 0, 0, 1]
    for i in (0, 1):
        cig.ops[i, :63] = (1 << 4) | 7
        cig.ops[i, 63] = (7 << 4) | 8
    cig.ops[5, 0] = (70 << 4) | 0
    ids = [b"ops%d" % i for i in range(6)]
    want, _ = snapgpu.bam_format(idx, reads, ids, res, cig, clip=clip)
    f = [fields(r) for r in split_records(want)]
    assert [len(x["ops"]) for x in f] == [66, 66, 2, 2, 0, 3]
    assert f[0]["ops"][0] == (2 << 4 | 4) and f[0]["ops"][-1] == (3 << 4 | 4) and f[1]["ops"][0] == (3 << 4 | 4)
    _same(aligner.bam_format(reads, ids, res, cig, clip=clip)[0], want)
    # unclipped, no ops at all on a mapped record: the span is the read's length
    reads2, ids2, res2, cig2 = made_up([pieces[0] + 7], [33], [0], n_ops=[0])
    want2, _ = snapgpu.bam_format(idx, reads2, ids2, res2, cig2, read_group=None)
    assert fields(split_records(want2)[0])["ops"] == []
    _same(aligner.bam_format(reads2, ids2, res2, cig2, read_group=None)[0], want2)


def test_records_that_pass_the_lds_window(aligner, idx, pieces):
    """40 reads of 500 bases with 200-byte ids: a workgroup's 32 records are some 32 KB, composed in
    several 16 KiB windows, unsorted and sorted (mapped in descending order, both directions, some
    unmapped that carry the NM before them; 1, 3 and 64 CIGAR ops)."""
    n = 40
    locs = [0xFFFFFFFF if i % 9 == 4 else pieces[1] + 50 + 3 * (n - i) for i in range(n)]
    ids = [b"%03d" % i + b"w" * 197 for i in range(n)]
    reads, ids, res, cig = made_up(locs, [500] * n, [i % 7 for i in range(n)], directions=[i & 1 for i in range(n)],
                                   ids=ids, n_ops=[(1, 3, 64)[i % 3] for i in range(n)])
    want, carry = snapgpu.bam_format(idx, reads, ids, res, cig, nm_carry=3)
    recs = split_records(want)
    assert len(recs) == n and all(fields(r)["lseq"] == 500 and len(fields(r)["name"]) == 200 for r in recs)
    assert sum(len(r) for r in recs[:GROUP]) > 16384
    got, got_carry = aligner.bam_format(reads, ids, res, cig, nm_carry=3)
    _same(got, want)
    assert got_carry == carry
    order = np.zeros(n, dtype=np.uint32)
    got, got_carry = aligner.bam_format(reads, ids, res, cig, nm_carry=3, sorted_output=True, order=order)
    assert np.array_equal(order, _key_order(idx, res)) and not np.array_equal(order, np.arange(n))
    assert sum(len(recs[int(i)]) for i in order[:GROUP]) > 16384
    _same(got, permuted(want, order))
    assert got_carry == carry


# ------------------------------------------------------------------------ NM carry
@pytest.fixture(scope="module")
def carry_case(pieces):
    """2 * TILE + 100 short reads: a mapped record (NM 3) at index 5, then unmapped records across the
    first tile's end and far into the second (a run longer than a tile that starts in one workgroup of
    the scan and of the write pass and ends in another), a mapped record (NM 6), unmapped to the end."""
    n = 2 * TILE + 100
    locs = np.full(n, 0xFFFFFFFF, dtype=np.uint64)
    locs[5] = pieces[0] + 100
    locs[TILE + TILE // 2 + 77] = pieces[1] + 40
    nm = np.zeros(n, dtype=np.int64)
    nm[5], nm[TILE + TILE // 2 + 77] = 3, 6
    return made_up(locs, [20] * n, nm)


def test_unmapped_run_across_tiles_and_workgroups(aligner, idx, carry_case):
    reads, ids, res, cig = carry_case
    want, carry = snapgpu.bam_format(idx, reads, ids, res, cig, nm_carry=5)
    nms = [fields(r)["nm"] for r in split_records(want)]
    cut = TILE + TILE // 2 + 77
    assert nms[:5] == [5] * 5 and set(nms[5:cut]) == {3} and set(nms[cut:]) == {6} and carry == 6
    got, got_carry = aligner.bam_format(reads, ids, res, cig, nm_carry=5)   # the batch starts unmapped
    _same(got, want)
    assert got_carry == 6


def test_all_unmapped_batch(aligner, idx):
    n = TILE + 3
    reads, ids, res, cig = made_up([0xFFFFFFFF] * n, [10] * n, [0] * n)
    for carry_in in (7, -1, 0):
        want, carry = snapgpu.bam_format(idx, reads, ids, res, cig, nm_carry=carry_in)
        got, got_carry = aligner.bam_format(reads, ids, res, cig, nm_carry=carry_in)
        _same(got, want)
        assert carry == got_carry == carry_in and fields(split_records(got)[-1])["nm"] == carry_in


def test_two_batches_chained_through_the_carry(world):
    """Two consecutive resident batches, the second seeded with the first's carry-out, equal one host
    call over both."""
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    half = 2000
    out, carry = b"", 11
    for start in (0, half):
        part = reads.slice(start, half)
        dev = al.upload(part)
        dev.run()
        dev.run_cigars()
        dev.run_bam(part, ids=ids[start:start + half], nm_carry=carry)
        carry = dev.bam_nm_carry()              # before bam(): waits on its own
        out += dev.bam()
        assert dev.bam_nm_carry() == carry
    want, want_carry = snapgpu.bam_format(world["idx"], reads, ids, world["res"], world["cig"], nm_carry=11)
    _same(out, want)
    assert carry == want_carry


# -------------------------------------------------------------------------- sorted
def test_resident_sorted_is_the_key_order_of_the_host_records(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    order = _key_order(world["idx"], world["res"])
    assert not np.array_equal(order, np.arange(reads.n))
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    dev.run_bam(reads, ids=ids, sorted_output=True)
    _same(dev.bam(), permuted(world["raw"], order))      # the carried NM values are those of input order
    assert np.array_equal(dev.bam_order(), order)
    assert dev.bam_nm_carry() == world["carry"]
    dev.run_bam(reads, ids=ids)                          # and unsorted again on the same state
    _same(dev.bam(), world["raw"])


@pytest.mark.parametrize("n", [1, 33, 1500, 5000])
def test_batch_sorted_fabricated_records(aligner, idx, fab, n):
    """Fabricated records, below and above rocPRIM's single-workgroup sort (1,024 pairs); carried NM
    values stay those of input order."""
    reads, ids, res, cig = fab
    reads, ids, res = reads.slice(0, n), ids[:n], res[:n]
    cig = snapgpu.Cigars(cig.editDistance[:n], cig.nOps[:n], cig.ops[:n])
    want, carry = snapgpu.bam_format(idx, reads, ids, res, cig, nm_carry=4)
    order = np.zeros(reads.n, dtype=np.uint32)
    got, got_carry = aligner.bam_format(reads, ids, res, cig, nm_carry=4, sorted_output=True, order=order)
    assert np.array_equal(order, _key_order(idx, res))
    _same(got, permuted(want, order))
    assert got_carry == carry


# ---------------------------------------------------------- buffers, ordering, errors
def test_buffer_reuse_growing_then_shrinking(world):
    al = world["aligner"]
    for start, n in ((0, 5), (7, 300), (100, 3900), (3999, 1), (0, 4000), (50, 64), (0, 0), (1234, 33)):
        reads, ids, res, cig = _slice(world, n, start)
        want, carry = snapgpu.bam_format(world["idx"], reads, ids, res, cig, nm_carry=1)
        for sorted_output in (False, True):
            got, got_carry = al.bam_format(reads, ids, res, cig, nm_carry=1, sorted_output=sorted_output)
            _same(got, permuted(want, _key_order(world["idx"], res)) if sorted_output else want)
            assert got_carry == carry, (start, n)


def test_resident_bam_ordered_before_next_run(world):
    """run(); run_cigars(); run_bam(); run(); bam() on one resident batch, 3 times: the BAM kernels read
    the records on the side stream, the next run's pre-fill and passes rewrite them and must wait."""
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = al.upload(reads)
    for _ in range(3):
        dev.run()
        dev.run_cigars()
        dev.run_bam(reads, ids=ids)
        dev.run()
        _same(dev.bam(), world["raw"])
    k, d = al.bam_ms()
    assert k > 0 and d > 0


def test_sam_and_bam_of_one_resident_batch(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    sam = snapgpu.sam_format(world["idx"], reads, ids, world["res"], world["cig"])
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    dev.run_sam(reads, ids=ids)
    dev.run_bam(reads, ids=ids)
    assert dev.sam() == sam
    _same(dev.bam(), world["raw"])
    dev.run_bam(reads, ids=ids, sorted_output=True)
    dev.run_sam(reads, ids=ids)
    _same(dev.bam(), permuted(world["raw"], _key_order(world["idx"], world["res"])))
    assert dev.sam() == sam
    with pytest.raises(snapgpu.SnapGpuError, match="not snapgpu_sam_resident_sorted"):
        dev.sam_order()                      # the sorted BAM call is not a sorted SAM call


def test_errors_raise_and_the_aligner_still_works(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = al.upload(reads)
    dev.run()
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_cigar_resident before"):
        dev.run_bam(reads, ids=ids)
    dev.run_cigars()
    with pytest.raises(snapgpu.SnapGpuError, match="does not match the resident batch"):
        dev.run_bam(reads.slice(0, reads.n - 1), ids=ids[:-1])
    with pytest.raises(snapgpu.SnapGpuError, match="no read ids"):
        dev.run_bam(reads)                   # a synthetic batch carries no ids
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_bam_resident before"):
        dev.bam()
    with pytest.raises(snapgpu.SnapGpuError, match="254"):
        dev.run_bam(reads, ids=[b"z" * 255] + ids[1:])
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_bam_resident before"):
        dev.bam()                            # the refused call left no state behind
    dev.run_bam(reads, ids=ids)
    with pytest.raises(snapgpu.SnapGpuError, match="not snapgpu_bam_resident_sorted"):
        dev.bam_order()
    # cap too small: non-zero, `used` set to the needed size
    used = C.c_uint64()
    buf = C.create_string_buffer(16)
    rc = snapgpu.lib().snapgpu_bam_download(al._h, dev._h, buf, 16, C.byref(used), None)
    assert rc != 0 and used.value == len(world["raw"]) and "too small" in snapgpu.last_error()
    _same(dev.bam(), world["raw"])
    with pytest.raises(snapgpu.SnapGpuError, match="254"):
        al.bam_format(reads.slice(0, 1), [b"z" * 255], world["res"][:1], _slice(world, 1)[3])
    with pytest.raises(snapgpu.SnapGpuError, match="no snapgpu_sam_resident before"):
        dev.sam()                            # SAM's state and messages are as they were
    r1, i1, s1, c1 = _slice(world, 10)
    _same(al.bam_format(r1, i1, s1, c1)[0], b"".join(world["recs"][:10]))
