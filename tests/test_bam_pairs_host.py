"""The paired BAM encoder on the host (snapgpu_bam_format_pairs over csrc/bam_pair_line.h; no GPU).

Against the reference: its own paired BAM records (both fixtures, '=' / 'X' and 'M' CIGARs) decoded
into encoder inputs (bam_pair_cases.fixture_runs) come back byte for byte, every record.  Against the
RNA paired path's encoder (bamAppendRecord with a mate, through
snapgpu_internal_bam_append_pair_records): the fabricated branches no fixture has.  Refusals, the
size contract, record lengths, the NM carry and its chaining, thread-count independence, sort keys."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import snapgpu
from bam_pair_cases import (PAIRS, VARIANTS, bam_fabricated, fixture_runs, python_sort_keys, record_fields, split_records,
                            unmapped_run_batch)
from sam_pair_cases import INVALID, PairBatch, _read, pair_results, small_index, too_long_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nm(raw):
    return [record_fields(r)["nm"] for r in split_records(raw)]


@pytest.mark.parametrize("stem,variant", VARIANTS)
def test_reference_records_come_back_byte_for_byte(stem, variant):
    """Every record of the fixture, none left out: per reference run, the carry 0 at its start."""
    index = small_index()
    records = unmapped = carried = 0
    for run in fixture_runs(stem, variant):
        carry = 0
        for batch, want in run:
            got, carry = snapgpu.bam_format_pairs(index, *batch.args(), nm_carry=carry)
            g, w = split_records(got), split_records(want)
            assert len(g) == len(w) == 2 * batch.n
            bad = [j for j in range(len(w)) if g[j] != w[j]]
            assert not bad, (len(bad), record_fields(g[bad[0]]), record_fields(w[bad[0]]))
            assert got == want
            records += len(w)
            f = [record_fields(r) for r in w]
            unmapped += sum(1 for x in f if x["flag"] & 0x4)
            carried += sum(1 for x in f if x["flag"] & 0x4 and x["nm"] != 0)
    # the fixtures hold what they are for: unmapped ends, some of which repeat an NM other than 0
    assert records == 2 * PAIRS[stem] and unmapped > 20 and carried > 5


def test_fixture_runs_reach_the_mate_branches():
    flags, other_piece, clipped = set(), 0, 0
    for run in fixture_runs("rna", ""):
        for _, want in run:
            for r in split_records(want):
                f = record_fields(r)
                flags.add(f["flag"] & 0xc)
                other_piece += f["refID"] >= 0 and f["next_refID"] >= 0 and f["refID"] != f["next_refID"]
                clipped += any(w & 15 == 4 for w in f["ops"])
    # (no pair of the fixtures is half mapped: the fabricated cases have those)
    assert flags == {0, 12} and other_piece > 0 and clipped > 50, (flags, other_piece, clipped)


@pytest.mark.parametrize("read_group", [None, "FASTQ", "g" * 300])
def test_fabricated_cases_equal_the_paired_writers_encoder(read_group):
    index = small_index()
    for batch, names in (bam_fabricated(), bam_fabricated(False)):
        for x, carry_in in ((batch, 0), (batch, 7), (batch.exchanged(), -3)):
            if x is not batch and batch is bam_fabricated()[0]:
                continue   # exchanged, the longest ids are not trimmed: refused (test_refusals)
            got, carry = snapgpu.bam_format_pairs(index, *x.args(), read_group=read_group, nm_carry=carry_in)
            want, want_carry = snapgpu._bam_append_pair_records(index, *x.args(), read_group=read_group, nm_carry=carry_in)
            g, w = split_records(got), split_records(want)
            assert len(g) == len(w) == 2 * batch.n
            for q, name in enumerate(names):
                assert g[2 * q:2 * q + 2] == w[2 * q:2 * q + 2], name
            assert carry == want_carry


def test_fabricated_cases_write_what_they_are_for():
    index = small_index()
    batch, names = bam_fabricated()
    raw, carry = snapgpu.bam_format_pairs(index, *batch.args())
    recs = [record_fields(r) for r in split_records(raw)]
    at = lambda name: recs[2 * names.index(name):2 * names.index(name) + 2]
    # NM -1 at a mapped end carries on over the three records behind it
    a, b = at("half mapped, NM -1 at the mapped end"), at("both unmapped after NM -1")
    assert [x["nm"] for x in a + b] == [-1, -1, -1, -1] and not a[0]["ops"] and not a[0]["flag"] & 0x4
    assert [x["nm"] for x in at("half mapped, end 1 mapped forward") + at("both unmapped after NM 4")] == [4, 4, 4, 4]
    # an unmapped end takes its mate's place, and the mate points at itself
    m, u = at("half mapped, end 1 mapped forward")
    assert (u["refID"], u["pos"], u["next_refID"], u["next_pos"]) == (m["refID"], m["pos"], m["refID"], m["pos"])
    assert (m["next_refID"], m["next_pos"]) == (m["refID"], m["pos"]) and m["flag"] & 0x8 and u["flag"] & 0x4
    assert u["bin"] == 4681 + (m["pos"] >> 14) and u["tlen"] == 0
    for x in at("both unmapped"):
        assert (x["refID"], x["pos"], x["next_refID"], x["next_pos"], x["bin"], x["tlen"]) == (-1, -1, -1, -1, 4680, 0)
    d = at("different pieces")
    assert d[0]["refID"] == d[1]["next_refID"] == 0 and d[0]["next_refID"] == d[1]["refID"] == 2 and d[0]["tlen"] == 0
    e = at("equal locations")
    assert e[0]["pos"] == e[1]["pos"] and e[0]["flag"] & 0x40 and not e[0]["flag"] & 0x10   # end 0 stays first
    f = at("64 ops and both soft clips")
    assert [len(x["ops"]) for x in f] == [66, 66] and f[0]["ops"][0] == (3 << 4 | 4) and f[0]["ops"][-1] == (4 << 4 | 4)
    assert f[1]["ops"][0] == (3 << 4 | 4) and f[1]["ops"][-1] == (2 << 4 | 4)   # mirrored for RC
    assert [x["l_seq"] for x in at("odd l_seq")] == [61, 1]
    assert at("deletion and skip widen the span")[0]["bin"] == 585   # 20 kb: a 128 kb bin
    assert [x["name"] for x in at("id with a space")] == [b"sp ace rest"] * 2
    assert [x["name"] for x in at("id with a space, no suffix")] == [b"na me"] * 2
    assert [len(x["name"]) for x in at("ids of 254 bytes after the trim") + at("ids of 254 bytes, no trim")] == [254] * 4
    low = at("lower case and N, odd")
    assert low[1]["seq"] == b"NNACGTR" * 9 and low[0]["seq"] == (b"NACGT" * 11)   # R is a BAM code of its own
    # before the first piece: no refID of its own, the mate's place in next_*
    p = at("before the first piece, mate mapped")
    assert (p[0]["refID"], p[0]["pos"]) == (-1, -1) and (p[0]["next_refID"], p[0]["next_pos"]) == (0, 50)
    assert carry == recs[-1]["nm"]


def test_refusals():
    index = small_index()
    batch, _ = bam_fabricated()
    r0, r1, res, cig = batch.args()
    rng = np.random.default_rng(1)
    a, b = _read(rng, 30), _read(rng, 30)

    def one(id0, id1):
        return PairBatch(([(id0, a[0], a[1])], [(id1, b[0], b[1])]), pair_results(1), [-1, -1], [[], []])

    snapgpu.bam_format_pairs(index, *one(b"q" * 254 + b"/1", b"q" * 254 + b"/2").args())
    for ids in ((b"q" * 255 + b"/1", b"q" * 255 + b"/2"), (b"q" * 255, b"short"), (b"q" * 253 + b"/2", b"q" * 253 + b"/1")):
        with pytest.raises(snapgpu.SnapGpuError, match="254"):
            snapgpu.bam_format_pairs(index, *one(*ids).args())
        with pytest.raises(snapgpu.SnapGpuError, match="254"):
            snapgpu.bam_pair_record_lengths(index, *one(*ids).args())
    with pytest.raises(snapgpu.SnapGpuError, match="254"):   # exchanged: "/2" "/1" stay, 256 bytes
        snapgpu.bam_format_pairs(index, *batch.exchanged().args())
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        snapgpu.bam_format_pairs(index, *too_long_batch().args())
    many = snapgpu.Cigars(cig.editDistance.copy(), cig.nOps.copy(), cig.ops.copy())
    many.nOps[7] = snapgpu._ffi.CIGAR_MAX_OPS + 1
    with pytest.raises(snapgpu.SnapGpuError, match="nOps"):
        snapgpu.bam_format_pairs(index, r0, r1, res, many)
    C = snapgpu.C
    used, carry = C.c_uint64(), C.c_int32()
    short = r1.slice(0, batch.n - 1)
    args = [res.ctypes.data, cig.editDistance.ctypes.data, cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ", 0, C.byref(carry)]
    fn = snapgpu.lib().snapgpu_bam_format_pairs
    assert fn(index._h, r0._p, short._p, *args, None, 0, C.byref(used)) == -1   # batches that differ in n
    # a short cap sets `used` and writes nothing; then the bytes suffice
    raw, _ = snapgpu.bam_format_pairs(index, r0, r1, res, cig)
    buf = C.create_string_buffer(b"\x7f" * len(raw), len(raw))
    assert fn(index._h, r0._p, r1._p, *args, buf, len(raw) - 1, C.byref(used)) == -1 and used.value == len(raw)
    assert buf.raw == b"\x7f" * len(raw)
    assert fn(index._h, r0._p, r1._p, *args, buf, len(raw), C.byref(used)) == 0 and buf.raw == raw


def test_record_lengths():
    index = small_index()
    batch, _ = bam_fabricated()
    for rg in (None, "FASTQ"):
        raw, _ = snapgpu.bam_format_pairs(index, *batch.args(), read_group=rg)
        lens = snapgpu.bam_pair_record_lengths(index, *batch.args(), read_group=rg)
        recs = split_records(raw)
        assert int(lens.sum()) == len(raw) and [len(r) for r in recs] == list(lens)
        assert all(int.from_bytes(r[:4], "little") + 4 == n for r, n in zip(recs, lens))


def test_nm_carry_chains():
    index = small_index()
    first = unmapped_run_batch(60, 0, 40)
    raw, carry = snapgpu.bam_format_pairs(index, *first.args(), nm_carry=7)
    assert _nm(raw)[:80] == [7] * 80 and _nm(raw)[80] == 7 + 40 and carry == _nm(raw)[-1]
    # the two halves of a batch, the carry passed on, are the whole
    batch, _ = bam_fabricated()
    whole, whole_carry = snapgpu.bam_format_pairs(index, *batch.args(), nm_carry=5)
    for cut in (1, 23, 24, batch.n - 1):   # 23 / 24: around the pair that leaves NM -1 behind
        halves, carry = b"", 5
        for a, b in ((0, cut), (cut, batch.n)):
            ids = [r.ids()[a:b] for r in batch.reads]
            ends = tuple([(ids[e][k], *_unclipped(batch, e, a + k)) for k in range(b - a)] for e in range(2))
            c = batch.cigars
            part = PairBatch(ends, batch.results[a:b], list(c.editDistance[2 * a:2 * b]),
                             [list(c.ops[j, :c.nOps[j]]) for j in range(2 * a, 2 * b)])
            raw, carry = snapgpu.bam_format_pairs(index, *part.args(), nm_carry=carry)
            halves += raw
        assert halves == whole and carry == whole_carry, cut
    empty = PairBatch(([], []), pair_results(0), [], [])
    assert snapgpu.bam_format_pairs(index, *empty.args(), nm_carry=12) == (b"", 12)


def _unclipped(batch, e, q):
    r = batch.reads[e]._p.contents
    front, full = int(batch.clips[e][0][q]), int(batch.clips[e][1][q])
    start = r.offsets[q] - front
    return snapgpu.C.string_at(r.bases + start, full), snapgpu.C.string_at(r.quals + start, full)


def thread_batch():
    """4,200 pairs (past the 8,192 records at which the host encoder takes more than one thread), a run
    of pairs unmapped on both ends across the cut between two threads' shares."""
    return unmapped_run_batch(4200, 2090, 2110)


def test_bytes_do_not_depend_on_the_thread_count():
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r); import snapgpu\n"
            "from test_bam_pairs_host import thread_batch\n"
            "from sam_pair_cases import small_index\n"
            "raw, carry = snapgpu.bam_format_pairs(small_index(), *thread_batch().args(), nm_carry=3)\n"
            "print(snapgpu.host_threads(), hashlib.sha256(raw).hexdigest(), len(raw), carry)"
            % (os.path.join(ROOT, "snap-rnaseq_amd"), os.path.join(ROOT, "tests")))
    outs = {}
    for threads in (1, 16):
        env = dict(os.environ, SNAPGPU_HOST_THREADS=str(threads))
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
        t, *rest = p.stdout.split()
        assert int(t) == threads
        outs[threads] = rest
    assert outs[1] == outs[16]
    # and they are the paired writer's
    batch = thread_batch()
    want, carry = snapgpu._bam_append_pair_records(small_index(), *batch.args(), nm_carry=3)
    assert outs[1] == [hashlib.sha256(want).hexdigest(), str(len(want)), str(carry)]


def test_sort_keys():
    index = small_index()
    for batch in (bam_fabricated()[0], bam_fabricated(False)[0].exchanged(), fixture_runs("rna", "")[0][0][0]):
        raw, _ = snapgpu.bam_format_pairs(index, *batch.args())
        keys = snapgpu.bam_pair_sort_keys(index, batch.results)
        want = python_sort_keys(index, split_records(raw))
        assert keys.dtype == np.uint32 and np.array_equal(keys, want)
    batch, names = bam_fabricated()
    keys = snapgpu.bam_pair_sort_keys(index, batch.results)
    q = names.index("before the first piece, mate mapped")
    assert keys[2 * q] == 500 + 50 == keys[2 * q + 1]          # own place invalid: the mate's
    q = names.index("both unmapped")
    assert list(keys[2 * q:2 * q + 2]) == [INVALID, INVALID]
    q = names.index("half mapped, end 1 RC")
    assert keys[2 * q] == keys[2 * q + 1] == 117293 + 7           # the unmapped end sorts with its mate
    assert len(snapgpu.bam_pair_sort_keys(index, pair_results(0))) == 0
