"""The paired SAM formatter on the host (snapgpu_sam_format_pairs) and the line rule the device runs
(csrc/sam_pair_line.h through its one-thread writer and its length pass), no GPU.

Reference pin without an aligner: the reference's own paired records (expected_rna_paired.sam.gz,
2,999 pairs; expected_rna150_paired.sam.gz, 2,000 pairs; the index of small.fa) are decoded back into
formatter inputs (sam_pair_cases.decode_fixture) and must come back byte for byte, every line of
every pair; with the two ends exchanged, the same bytes wherever the locations differ.

No fixture of the reference has a half-mapped pair (its filter never emits one): that branch, and
the others the fixtures miss, are fabricated; there the line rule is held to the product path's own
line writer (samAppendLine with SamLine::hasMate, which snapgpu_sam_format_pairs runs) and to a
plain-Python restatement of the rule."""
import numpy as np
import pytest

import snapgpu
from sam_pair_cases import (FIXTURES, INVALID, decode_fixture, fabricated, python_lines, small_index, split_lines,
                            too_long_batch)


@pytest.mark.parametrize("stem", sorted(FIXTURES))
def test_reference_records_come_back_byte_for_byte(stem):
    index = small_index()
    batch, lines, counts = decode_fixture(stem)
    assert batch.n == FIXTURES[stem] and len(lines) == 2 * batch.n   # no pair is left out
    got = split_lines(snapgpu.sam_format_pairs(index, *batch.args()))
    assert len(got) == len(lines)
    bad = [j for j in range(len(lines)) if got[j] != lines[j]]
    assert not bad, (len(bad), got[bad[0]], lines[bad[0]])
    # the line rule's own writer and the plain restatement print the same
    assert split_lines(snapgpu._sam_pair_line_write(index, *batch.args())) == lines
    assert python_lines(index, batch) == lines
    lens = snapgpu.sam_pair_line_lengths(index, *batch.args())
    assert lens.tolist() == [len(l) for l in lines]


@pytest.mark.parametrize("stem", sorted(FIXTURES))
def test_ids_with_their_suffixes_give_the_same_records(stem):
    """The writer dropped "/1" and "/2" from the ids: given back, they are dropped again."""
    batch, lines, _ = decode_fixture(stem, True)
    assert batch.reads[0].ids()[0].endswith(b"/1") and batch.reads[1].ids()[0].endswith(b"/2")
    assert split_lines(snapgpu.sam_format_pairs(small_index(), *batch.args())) == lines


@pytest.mark.parametrize("stem", sorted(FIXTURES))
def test_exchanged_ends_give_the_same_bytes_where_the_locations_differ(stem):
    index = small_index()
    batch, lines, _ = decode_fixture(stem)
    got = split_lines(snapgpu.sam_format_pairs(index, *batch.exchanged().args()))
    loc = np.where(batch.results["status"] != snapgpu.NotFound, batch.results["location"], INVALID)
    differ = loc[:, 0] != loc[:, 1]
    assert differ.sum() > batch.n // 2 and (~differ).sum() > 100
    for q in range(batch.n):
        same = got[2 * q:2 * q + 2] == lines[2 * q:2 * q + 2]
        assert same or not differ[q], q
        if loc[q, 0] == INVALID and loc[q, 1] == INVALID:   # equal locations keep end 0 first: the lines change places
            flip = lambda l, a, b: l.replace(b"\t%d\t" % a, b"\t%d\t" % b, 1)
            assert got[2 * q] == flip(lines[2 * q + 1], 141, 77) and got[2 * q + 1] == flip(lines[2 * q], 77, 141), q


def test_fixtures_carry_what_they_are_for():
    _, lines, counts = decode_fixture("rna")
    assert counts["flags"] == {67, 131, 83, 163, 99, 147, 115, 179, 77, 141}
    assert counts["other_piece"] == 318 and counts["n_ops"] == 163 and counts["max_ops"] == 29
    # 222 pairs carry a soft clip, always on one end only: on the first written line in 118 of them, on
    # the second in 104
    assert counts["soft_clipped_pairs"] == 222 and counts["soft_clipped_first"] == 118
    # no half-mapped pair, no mapped end without CIGAR
    for stem in FIXTURES:
        b, _, _ = decode_fixture(stem)
        st = b.results["status"] != snapgpu.NotFound
        assert (st[:, 0] == st[:, 1]).all()
        assert (b.cigars.editDistance.reshape(-1, 2)[st] >= 0).all()


@pytest.mark.parametrize("read_group", ["FASTQ", None, "g" * 300])
def test_fabricated_cases(read_group):
    index = small_index()
    batch, names = fabricated()
    got = split_lines(snapgpu.sam_format_pairs(index, *batch.args(), read_group=read_group))
    rule = split_lines(snapgpu._sam_pair_line_write(index, *batch.args(), read_group=read_group))
    plain = python_lines(index, batch, read_group)
    assert len(got) == 2 * batch.n
    for q, name in enumerate(names):
        assert got[2 * q:2 * q + 2] == rule[2 * q:2 * q + 2], name
        assert got[2 * q:2 * q + 2] == plain[2 * q:2 * q + 2], name
    lens = snapgpu.sam_pair_line_lengths(index, *batch.args(), read_group=read_group)
    assert lens.tolist() == [len(l) for l in got]
    tag = b"" if read_group is None else b"\tRG:Z:" + read_group.encode()
    assert all(l.count(b"\tRG:Z:") == (read_group is not None) and tag in l for l in got)


def test_fabricated_cases_print_what_they_are_for():
    batch, names = fabricated()
    got = [l.split(b"\t") for l in split_lines(snapgpu.sam_format_pairs(small_index(), *batch.args()))]
    pair = lambda name: got[2 * names.index(name):2 * names.index(name) + 2]
    a, b = pair("half mapped, end 0")       # the mapped end first; the unmapped one takes its RNAME and POS
    assert a[:9] == [b"h0", b"73", b"chr1", b"101", b"60", b"60=", b"=", b"101", b"0"]
    assert b[:9] == [b"h0", b"133", b"chr1", b"101", b"0", b"*", b"=", b"101", b"0"] and b[-1] == b"NM:i:-1\n"
    a, b = pair("half mapped, end 1 RC")    # 0x10 on the mapped end, 0x20 on its mate
    assert (a[1], b[1], a[2], b[2], b[3]) == (b"89", b"165", b"chr2", b"chr2", b"8")
    a, b = pair("half mapped, stale location")   # a NotFound end's location counts for nothing
    assert (a[1], a[2], b[1], b[5]) == (b"73", b"chr3", b"133", b"*")
    a, b = pair("both unmapped")
    assert a[1:9] == [b"77", b"*", b"0", b"0", b"*", b"=", b"0", b"0"] and b[1] == b"141"
    a, b = pair("equal locations")          # end 0 stays first
    assert (a[1], b[1]) == (b"99", b"147")
    a, b = pair("end 1 lower")
    assert (a[1], a[3], b[1], b[3], a[8], b[8]) == (b"99", b"8801", b"147", b"9001", b"260", b"-260")
    a, b = pair("different pieces")
    assert (a[6], a[7], a[8], b[6], b[7], b[8]) == (b"chr3", b"70001", b"0", b"chr1", b"11", b"0")
    a, b = pair("negative and long TLEN")
    assert (a[8], b[8]) == (b"116060", b"-116060")
    a, b = pair("different clips")          # TLEN spans the unclipped reads: 701 + 66 - 501 - ... of both clip states
    assert (a[5], b[5], a[8], b[8]) == (b"3S30=1X36=", b"5S20=2I37=2S", b"264", b"-264")
    a, b = pair("MAPQ above 70 and below 0")
    assert (a[4], b[4]) == (b"70", b"0")
    assert [l[0] for l in pair("ids /2 /1")] == [b"x/2", b"x/1"]   # the condition's (c0 == '1' || c1 == '2') term
    assert [l[0] for l in pair("ids /1 /1")] == [b"y/1", b"y/1"]
    assert [l[0] for l in pair("ids of unequal length")] == [b"long-name/1", b"nm/2"]
    assert [l[0] for l in pair("space before the suffix")] == [b"sp", b"sp"]
    assert [l[0] for l in pair("suffix only")] == [b"/1", b"/2"]
    a, b = pair("a base that complements to NUL")
    assert len(a[9]) == 60 and len(b[9]) == 19 and len(b[10]) == 60
    a, b = pair("mapped without CIGAR")
    assert (a[5], a[-1]) == (b"*", b"NM:i:-1\n")
    assert pair("a full row of ops")[0][5] == b"1=1X" * 32


def test_refusals():
    index = small_index()
    batch, _ = fabricated()
    r0, r1, res, cig = batch.args()
    with pytest.raises((snapgpu.SnapGpuError, ValueError)):
        snapgpu.sam_format_pairs(index, r0, r1.slice(0, batch.n - 1), res, cig)
    long_one = too_long_batch()
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        snapgpu.sam_format_pairs(index, *long_one.args())
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        snapgpu.sam_pair_line_lengths(index, *long_one.args())
    many = snapgpu.Cigars(cig.editDistance.copy(), cig.nOps.copy(), cig.ops.copy())
    many.nOps[5] = snapgpu._ffi.CIGAR_MAX_OPS + 1
    with pytest.raises(snapgpu.SnapGpuError, match="nOps"):
        snapgpu.sam_format_pairs(index, r0, r1, res, many)
    # the C call itself refuses batches that differ in n, and follows the size contract
    C = snapgpu.C
    used = C.c_uint64()
    short = r1.slice(0, batch.n - 1)
    args = [res.ctypes.data, cig.editDistance.ctypes.data, cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ"]
    fn = snapgpu.lib().snapgpu_sam_format_pairs
    assert fn(index._h, r0._p, short._p, *args, None, 0, C.byref(used)) == -1
    assert "differ" in snapgpu.last_error()
    assert fn(index._h, r0._p, r1._p, *args, None, 0, C.byref(used)) == -1
    text = snapgpu.sam_format_pairs(index, r0, r1, res, cig)
    assert used.value == len(text)
    buf = C.create_string_buffer(len(text))
    assert fn(index._h, r0._p, r1._p, *args, buf, len(text) - 1, C.byref(used)) == -1
    assert fn(index._h, r0._p, r1._p, *args, buf, len(text), C.byref(used)) == 0 and buf.raw == text


def test_batches_past_the_thread_threshold():
    """4,500 pairs (the formatter splits batches of 4,096 pairs or more over the host threads): random
    records over clipped synthetic reads, the threaded writer against the line rule's own."""
    from sam_pair_cases import pair_results, synthetic_batch
    index = small_index()
    n = 4500
    r0, r1 = synthetic_batch(index.genome_handle(), n, True, seed=3)
    rng = np.random.default_rng(3)
    res = pair_results(n)
    res["status"] = rng.integers(0, 3, (n, 2))
    res["location"] = rng.integers(500, 300000, (n, 2))
    res["direction"] = rng.integers(0, 2, (n, 2))
    res["mapq"] = rng.integers(0, 71, (n, 2))
    cig = snapgpu.Cigars.empty(2 * n)
    cig.editDistance[:] = rng.integers(-1, 9, 2 * n)
    cig.nOps[:] = rng.integers(0, 6, 2 * n)
    cig.ops[:, :6] = (rng.integers(1, 90, (2 * n, 6)) << 4) | rng.integers(0, 9, (2 * n, 6))
    got = snapgpu.sam_format_pairs(index, r0, r1, res, cig)
    assert got == snapgpu._sam_pair_line_write(index, r0, r1, res, cig)
    assert got.count(b"\n") == 2 * n
    assert snapgpu.sam_pair_line_lengths(index, r0, r1, res, cig).sum() == len(got)
