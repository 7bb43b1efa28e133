"""Coordinate-sorted SAM text from the device formatter (`-so`; csrc/sam_format.hip: the length pass
stores each record's sort key, rocprim::radix_sort_pairs orders (key, record), the scan and the
write pass run over output slots).  The expectation is always the host sorter over the unsorted
text -- snapgpu_sam_sort_records, pinned to the reference by test_sorted.py -- and the stable
argsort of snapgpu_sam_sort_keys for the order itself; the unsorted device text is pinned to the
reference by test_sam_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import snapgpu
from sam_cases import G, READ_GROUPS, fabricated_case, fastq, small_index
from sam_sort_cases import key_order, reorder, six_contig_index

pytestmark = pytest.mark.gpu

# rocPRIM's radix_sort_pairs (device_radix_sort.hpp, radix_sort_impl) sorts up to 1,024 pairs of
# 32-bit keys and values in a single workgroup (256 threads x 4 items); above that, and up to its
# merge_sort_limit of 1,048,576, it merges block-sorted runs; larger inputs take the onesweep radix
# passes.  N_BIG is far past the first threshold; the sizes below also straddle it.
ROCPRIM_SINGLE_WORKGROUP_PAIRS = 1024
N_BIG = 20_000


@pytest.fixture(scope="module")
def genomes(gpu_available, tmp_path_factory):
    """The two genomes of the batch-form tests, each with its aligner."""
    small, six = small_index(), six_contig_index(tmp_path_factory.mktemp("six"))
    return {"small": (small, snapgpu.BaseAligner(small)), "six": (six, snapgpu.BaseAligner(six))}


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    """small_world's 4,000 reads with ids, aligned once on the device: records, CIGARs, the host
    formatter's line of every read and one aligner, shared by the tests below and never modified."""
    idx, reads = small_world["index"], small_world["reads"]
    al = snapgpu.BaseAligner(idx)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    res, cig = dev.results(), dev.cigars()
    ids = [b"read_%d extra" % i for i in range(reads.n)]
    lines = snapgpu.sam_format(idx, reads, ids, res, cig).splitlines(keepends=True)
    assert len(lines) == reads.n
    v = idx.view()
    pieces = [int(x) for x in C.cast(v.pieceOffsets, C.POINTER(C.c_uint32))[:v.nPieces]]
    return dict(idx=idx, reads=reads, res=res, cig=cig, ids=ids, lines=lines, aligner=al, pieces=pieces)


def _slice(world, n, start=0):
    c = snapgpu.Cigars(world["cig"].editDistance[start:start + n], world["cig"].nOps[start:start + n],
                       world["cig"].ops[start:start + n])
    return (world["reads"].slice(start, n), world["ids"][start:start + n], world["res"][start:start + n], c,
            b"".join(world["lines"][start:start + n]))


def _check_batch(idx, al, reads, ids, res, cig, unsorted, **kw):
    """The sorted batch call against the host sorter over `unsorted` and against the key order."""
    text, order = al.sam_format(reads, ids, res, cig, sorted_output=True, return_order=True, **kw)
    assert np.array_equal(np.sort(order), np.arange(reads.n))   # a permutation
    assert np.array_equal(order, key_order(idx, res))
    assert text == snapgpu.sam_sort_records(idx, unsorted)
    return text, order


# ------------------------------------------------------------------ resident chain
@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clip3"])
@pytest.mark.parametrize("use_m", [0, 1])
def test_resident_sorted_is_host_sort_of_unsorted(genomes, use_m, clip):
    idx, al = genomes["small"]
    reads = snapgpu.Reads.from_fastq(os.path.join(G, "small_reads.fq"))
    if clip:
        reads.clip(3)
    ids = [i for i, _, _ in fastq(os.path.join(G, "small_reads.fq"))]
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars(useM=use_m)
    dev.run_sam(reads, ids=ids)
    unsorted = dev.sam()
    dev.run_sam(reads, ids=ids, sorted_output=True)
    got = dev.sam()
    assert got == snapgpu.sam_sort_records(idx, unsorted)
    assert got != unsorted
    assert np.array_equal(dev.sam_order(), key_order(idx, dev.results()))


# ---------------------------------------------------------------------- batch form
@pytest.mark.parametrize("read_group", READ_GROUPS)
@pytest.mark.parametrize("genome", ["small", "six"])
def test_batch_sorted_fabricated_records(genomes, genome, read_group):
    idx, al = genomes[genome]
    reads, ids, res, cig, _ = fabricated_case(idx)
    unsorted = snapgpu.sam_format(idx, reads, ids, res, cig, read_group=read_group)
    text, _ = _check_batch(idx, al, reads, ids, res, cig, unsorted, read_group=read_group)
    assert text != unsorted


# ------------------------------------------------------ ties and degenerate orders
def _made_up(world, locations):
    """One 70-base read per entry of `locations` (0xffffffff: NotFound) with CIGAR "*" -> batch inputs."""
    n = len(locations)
    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGT"), size=70)) for _ in range(4)]
    reads = snapgpu.Reads.from_list([(seqs[i % 4], "I" * 70) for i in range(n)])
    res = np.zeros(n, dtype=snapgpu.RESULT_DTYPE)
    res["location"] = np.asarray(locations, dtype=np.uint32)
    res["result"] = np.where(res["location"] == 0xFFFFFFFF, snapgpu.NotFound, snapgpu.SingleHit)
    res["mapq"] = 30
    ids = [b"t%d" % i for i in range(n)]
    cig = snapgpu.Cigars.empty(n)
    return reads, ids, res, cig, snapgpu.sam_format(world["idx"], reads, ids, res, cig)


def test_ties_keep_input_order(world):
    """300 copies of one mapped location interleaved with 300 unmapped records: two groups of equal
    keys, each in input order (the radix sort is stable, as std::stable_sort is)."""
    loc = np.full(600, 0xFFFFFFFF, dtype=np.uint64)
    loc[0::2] = world["pieces"][1] + 1234
    reads, ids, res, cig, unsorted = _made_up(world, loc)
    _, order = _check_batch(world["idx"], world["aligner"], reads, ids, res, cig, unsorted)
    assert order.tolist() == list(range(0, 600, 2)) + list(range(1, 600, 2))


def test_all_unmapped_keeps_input_order(world):
    reads, ids, res, cig, unsorted = _made_up(world, np.full(600, 0xFFFFFFFF, dtype=np.uint64))
    text, order = _check_batch(world["idx"], world["aligner"], reads, ids, res, cig, unsorted)
    assert order.tolist() == list(range(600)) and text == unsorted


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_keys_already_ordered(world, descending):
    """Keys ascending (nothing moves) and strictly descending (everything does), across two pieces."""
    p = world["pieces"]
    loc = np.concatenate([p[0] + 10 + 7 * np.arange(300), p[2] + 10 + 7 * np.arange(300)])
    reads, ids, res, cig, unsorted = _made_up(world, loc[::-1] if descending else loc)
    text, order = _check_batch(world["idx"], world["aligner"], reads, ids, res, cig, unsorted)
    assert order.tolist() == (list(range(599, -1, -1)) if descending else list(range(600)))
    assert (text == unsorted) == (not descending)


# --------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [0, 1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4000])
def test_batch_sizes(world, n):
    """Around the wave, the write pass's 32 slots per workgroup and the scan tile; 0 .. 65 stay in
    rocPRIM's single-workgroup sort, 2047 and up leave it."""
    reads, ids, res, cig, unsorted = _slice(world, n)
    _check_batch(world["idx"], world["aligner"], reads, ids, res, cig, unsorted)


def test_big_batch_leaves_the_single_workgroup_sort(genomes):
    assert N_BIG > ROCPRIM_SINGLE_WORKGROUP_PAIRS
    idx, al = genomes["six"]
    reads, ids, res, cig, _ = fabricated_case(idx, n=N_BIG, seed=7)
    unsorted = snapgpu.sam_format(idx, reads, ids, res, cig)
    _check_batch(idx, al, reads, ids, res, cig, unsorted)


# -------------------------------------------------------------------- buffer reuse
def test_buffer_reuse_growing_then_shrinking(world):
    """One aligner's grow-only buffers (keys, orders, sort storage) over growing, then shrinking n,
    with an unsorted call between sorted ones."""
    al = world["aligner"]
    for start, n in ((0, 5), (7, 300), (100, 3900), (3999, 1), (0, 4000), (50, 64), (0, 0), (1234, 33)):
        reads, ids, res, cig, unsorted = _slice(world, n, start)
        _check_batch(world["idx"], al, reads, ids, res, cig, unsorted)
        assert al.sam_format(reads, ids, res, cig) == unsorted, (start, n)


def test_resident_alternating_sorted_and_unsorted(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    unsorted = b"".join(world["lines"])
    want = snapgpu.sam_sort_records(world["idx"], unsorted)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    for sorted_output in (True, False, True, True, False):
        dev.run_sam(reads, ids=ids, sorted_output=sorted_output)
        assert dev.sam() == (want if sorted_output else unsorted), sorted_output
    dev.run_sam(reads, ids=ids, sorted_output=True)
    assert np.array_equal(dev.sam_order(), key_order(world["idx"], world["res"]))


# -------------------------------------------------------------- ordering across runs
def test_resident_sorted_sam_ordered_before_next_run(world):
    """run(); run_cigars(); run_sam(sorted); run(); sam() on one resident batch, 3 times: the next
    run's pre-fill and passes rewrite the records the sorted SAM kernels read, and must wait."""
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    want = snapgpu.sam_sort_records(world["idx"], b"".join(world["lines"]))
    dev = al.upload(reads)
    for _ in range(3):
        dev.run()
        dev.run_cigars()
        dev.run_sam(reads, ids=ids, sorted_output=True)
        dev.run()
        assert dev.sam() == want


# ------------------------------------------------------------------ tab in a QNAME
def test_tab_in_a_qname_follows_the_records_key(world):
    """A QNAME with a tab shifts every field of its line for a parser: the host sorter then reads
    FLAG as RNAME and RNAME as POS, finds no such contig and no digits, and gives the line key
    0 + 0 - 1 = 0xffffffff, so it sorts the record behind every mapped one.  The device takes the key
    from the record itself, so the line stays at its coordinate; the two texts differ."""
    idx, al = world["idx"], world["aligner"]
    reads, ids, res, cig, _ = _slice(world, 200)
    keys = snapgpu.sam_sort_keys(idx, res)
    first = int(np.argmin(keys))
    assert keys[first] != 0xFFFFFFFF and (keys > keys[first]).any()
    ids = list(ids)
    ids[first] = b"tab\tbed name"
    unsorted = snapgpu.sam_format(idx, reads, ids, res, cig)
    text, order = al.sam_format(reads, ids, res, cig, sorted_output=True, return_order=True)
    assert np.array_equal(order, key_order(idx, res))
    assert text == reorder(unsorted, order)
    assert text.startswith(b"tab\tbed\t")
    assert snapgpu.sam_sort_records(idx, unsorted) != text


# -------------------------------------------------------------------------- errors
def test_errors_and_the_aligner_still_works(world):
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    with pytest.raises(snapgpu.SnapGpuError, match="not snapgpu_sam_resident_sorted"):
        dev.sam_order()                       # no run_sam yet
    dev.run_sam(reads, ids=ids)
    with pytest.raises(snapgpu.SnapGpuError, match="not snapgpu_sam_resident_sorted"):
        dev.sam_order()                       # the last one was unsorted
    unsorted = dev.sam()
    assert al.sam_sort_ms() == 0
    dev.run_sam(reads, ids=ids, sorted_output=True)
    want = snapgpu.sam_sort_records(world["idx"], unsorted)
    assert dev.sam() == want
    assert al.sam_sort_ms() > 0
    length, scan, write = al.sam_pass_ms()
    kernel, _ = al.sam_ms()
    assert min(length, scan, write) > 0 and length + scan + write + al.sam_sort_ms() <= kernel * 1.001
    with pytest.raises(ValueError, match="return_order needs sorted_output"):
        al.sam_format(*_slice(world, 3)[:4], return_order=True)
    assert np.array_equal(dev.sam_order(), key_order(world["idx"], world["res"]))
