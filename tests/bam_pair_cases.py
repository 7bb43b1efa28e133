"""Shared inputs of the paired BAM encoder tests (test_bam_pairs_host.py, test_bam_pairs_gpu.py).

fixture_runs(): the reference's own paired BAM records (expected_{rna,rna150}_paired{,_M}.bam.records.gz,
written on the index of small.fa) decoded back into the encoder's inputs, per reference run (the NM
carry starts at 0 in each).  Everything comes from the BAM records themselves: ids, reads
(SEQ and QUAL turned back for RC ends), the clip state (Read::clip of the decoded qualities, checked
against the soft clips), pair records and CIGAR rows.  bam_fabricated(): sam_pair_cases.fabricated()
with the branches only BAM has.  split_records / record_fields / python_sort_keys: the record layout
and BAMFormat::getSortInfo in plain Python."""
import ctypes
import functools
import gzip
import json
import os
import struct

import numpy as np

import snapgpu
from sam_pair_cases import (G, INVALID, PairBatch, _read, fabricated, index_pieces, pair_results, revcomp,
                            small_index)

SEQ_CODES = "=ACMGRSVTWYHKDBN"
VARIANTS = [("rna", ""), ("rna", "_M"), ("rna150", ""), ("rna150", "_M")]
PAIRS = {"rna": 2999, "rna150": 2000}


def split_records(raw):
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<i", raw, at)[0] + 4
        out.append(raw[at:at + size])
        at += size
    assert at == len(raw)
    return out


def record_fields(rec):
    """One BAM record -> dict of its fixed fields, name, ops, seq, qual (phred + 33) and NM."""
    block, ref, pos, lname, mapq, bin_, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    assert block + 4 == len(rec)
    at = 36
    name = rec[at:at + lname - 1]
    assert rec[at + lname - 1] == 0
    at += lname
    ops = list(struct.unpack_from(f"<{ncig}I", rec, at))
    at += 4 * ncig
    packed = rec[at:at + (lseq + 1) // 2]
    at += (lseq + 1) // 2
    seq = "".join(SEQ_CODES[b >> 4] + SEQ_CODES[b & 15] for b in packed)[:lseq].encode()
    qual = bytes(q + 33 for q in rec[at:at + lseq])
    at += lseq
    tags = rec[at:]
    assert tags[-7:-4] == b"NMi"
    return dict(refID=ref, pos=pos, mapq=mapq, bin=bin_, flag=flag, l_seq=lseq, next_refID=nref, next_pos=npos,
                tlen=tlen, name=name, ops=ops, seq=seq, qual=qual, nm=struct.unpack("<i", tags[-4:])[0], tags=tags[:-7])


def block_sizes(stem):
    """Pairs per reference run, in order (the NM carry starts at 0 in each run)."""
    if stem == "rna":
        n = PAIRS[stem]
        return [min(200, n - a) for a in range(0, n, 200)]
    return json.load(open(os.path.join(G, f"expected_{stem}_blocks.json")))["block_sizes"]


def piece_starts(index):
    return [int(o) for _, o in index_pieces(index)]


@functools.lru_cache(maxsize=None)
def fixture_runs(stem, variant):
    """-> per reference run a list of (PairBatch, record bytes of its records) that follow one
    another: the NM carry starts at 0 in each run and passes from one batch of a run to the next.
    The first record of a pair is taken as end 0: it is the end at the lower (or equal) location,
    which the rule writes first.  The ids get back the "/1" and "/2" the writer dropped.

    A run is one batch, clipped by Read::clip of the decoded qualities as the reference's reader clipped
    it; a record's CIGAR row is its ops without the soft clips that clip state explains.  The
    reference counts an uninitialised slot behind the ops of some transcriptome records in
    n_cigar_op; that word is kept in the row, as it is in the record.  Where it lies behind a soft
    clip no row can hold it: such a pair becomes a batch of its own, unclipped, both rows the
    records' ops as they are (TLEN is the same as long as neither end is clipped before its
    location)."""
    starts = piece_starts(small_index())
    raw = gzip.open(os.path.join(G, f"expected_{stem}_paired{variant}.bam.records.gz"), "rb").read()
    recs = split_records(raw)
    assert len(recs) == 2 * PAIRS[stem]
    runs, at = [], 0
    for size in block_sizes(stem):
        part = recs[2 * at:2 * (at + size)]
        at += size
        results = pair_results(size)
        ends = ([], [])
        fields = [record_fields(rec) for rec in part]
        for j, f in enumerate(fields):
            q, e = divmod(j, 2)
            assert f["flag"] & (0x40 if e == 0 else 0x80) and f["tags"] == b"RGZFASTQ\0PGZSNAP\0"
            rc, mapped = bool(f["flag"] & 0x10), not f["flag"] & 0x4
            if mapped:
                results["status"][q, e] = snapgpu.SingleHit if f["mapq"] > 10 else snapgpu.MultipleHits
                results["location"][q, e] = starts[f["refID"]] + f["pos"]
                results["direction"][q, e] = int(rc)
                results["mapq"][q, e] = f["mapq"]
            else:
                assert not rc and not f["ops"]
            name = f["name"] + (b"/1", b"/2")[e]
            ends[e].append((name, revcomp(f["seq"]) if rc else f["seq"], f["qual"][::-1] if rc else f["qual"]))
        probe = PairBatch(ends, results, [-1] * (2 * size), [[]] * (2 * size))   # for Read::clip's state
        ed, rows, whole, alone = [], [], [], set()
        for j, f in enumerate(fields):
            q, e = divmod(j, 2)
            mapped = not f["flag"] & 0x4
            front, full = int(probe.clips[e][0][q]), int(probe.clips[e][1][q])
            back = full - int(probe.reads[e].lengths()[q]) - front
            before, after = (back, front) if f["flag"] & 0x10 else (front, back)
            row = list(f["ops"]) if mapped and f["nm"] >= 0 else []
            assert mapped or not f["ops"]
            whole.append(list(row))
            if row and before:
                if row[0] != (before << 4 | 4):
                    alone.add(q)
                row = row[1:]
            if row and after:
                if row[-1] != (after << 4 | 4):
                    alone.add(q)
                row = row[:-1]
            ed.append(f["nm"] if mapped else -1)
            rows.append(row)
        run, a = [], 0
        for q in sorted(alone) + [size]:
            if q > a:
                run.append((PairBatch(tuple(x[a:q] for x in ends), results[a:q], ed[2 * a:2 * q], rows[2 * a:2 * q]),
                            b"".join(part[2 * a:2 * q])))
            if q < size:
                run.append((PairBatch(tuple(x[q:q + 1] for x in ends), results[q:q + 1], ed[2 * q:2 * q + 2],
                                      whole[2 * q:2 * q + 2], clipping=None), b"".join(part[2 * q:2 * q + 2])))
            a = q + 1
        assert sum(b.n for b, _ in run) == size and len(alone) <= 1
        runs.append(run)
    assert at == PAIRS[stem]
    return runs


@functools.lru_cache(maxsize=None)
def bam_fabricated(longest_ids=True):
    """-> (PairBatch, [case name per pair]): sam_pair_cases.fabricated()'s pairs, then the branches
    only the BAM record has.  The order matters for the NM carry: the pair mapped without CIGAR
    (NM -1) is followed by a pair with both ends unmapped.  longest_ids False: the ids of 254 bytes
    after the trim are 200 bytes instead (with the ends exchanged they are "/2" "/1", which
    writePair does not trim: 256 bytes, refused)."""
    base, names = fabricated()
    rng = np.random.default_rng(24)
    chr1, chr2, chr3 = 500, 117293, 230679
    S, M, NF, F, R = snapgpu.SingleHit, snapgpu.MultipleHits, snapgpu.NotFound, snapgpu.FORWARD, snapgpu.RC
    eq = lambda n: [(n << 4) | 7]
    r = lambda n=60, f=0, b=0: _read(rng, n, f, b)
    cases = []

    def add(name, ids, reads, e0, e1):
        cases.append((name, ids, reads, (e0, e1)))

    un = (NF, INVALID, F, 0, -1, [])
    add("half mapped, NM -1 at the mapped end", (b"q0/1", b"q0/2"), (r(), r()), (S, chr2 + 40, R, 10, -1, []), un)
    add("both unmapped after NM -1", (b"q1/1", b"q1/2"), (r(), r()), un, (NF, chr1 + 9, R, 3, 5, eq(60)))
    add("half mapped, end 1 mapped forward", (b"q2/1", b"q2/2"), (r(), r()), un, (M, chr3 + 11, F, 7, 4, eq(60)))
    add("both unmapped after NM 4", (b"q3/1", b"q3/2"), (r(), r()), un, un)
    add("before the first piece, mate mapped", (b"q4/1", b"q4/2"), (r(), r()), (S, 100, F, 30, 1, eq(60)), (S, chr1 + 50, R, 31, 0, eq(60)))
    add("before the first piece, mate unmapped", (b"q5/1", b"q5/2"), (r(), r()), un, (S, 7, R, 30, 2, eq(60)))
    add("64 ops and both soft clips", (b"q6/1", b"q6/2"), (r(71, 3, 4), r(69, 2, 3)),
        (S, chr2 + 5000, F, 10, 30, [(1 << 4) | (7 + (k & 1)) for k in range(64)]),
        (S, chr2 + 5200, R, 10, 31, [(1 << 4) | (7 + (k & 1)) for k in range(64)]))
    add("odd l_seq", (b"q7/1", b"q7/2"), (r(61), r(1)), (S, chr1 + 700, F, 10, 0, eq(61)), (S, chr1 + 900, R, 10, 0, eq(1)))
    add("deletion and skip widen the span", (b"q8/1", b"q8/2"), (r(), r()),
        (S, chr1 + 16000, F, 10, 3, [(30 << 4) | 7, (20000 << 4) | 3, (30 << 4) | 7]),
        (S, chr1 + 16300, R, 10, 3, [(30 << 4) | 7, (3 << 4) | 2, (30 << 4) | 7]))
    add("id with a space", (b"sp ace rest/1", b"sp ace rest/2"), (r(), r()), (S, chr1 + 23, F, 1, 0, eq(60)), (S, chr1 + 303, R, 1, 0, eq(60)))
    add("id with a space, no suffix", (b"na me", b"na me"), (r(), r()), (S, chr1 + 24, F, 1, 0, eq(60)), un)
    long_id = b"L" * (254 if longest_ids else 200)
    add("ids of 254 bytes after the trim", (long_id + b"/1", long_id + b"/2"), (r(), r()), (S, chr3 + 900, R, 1, 0, eq(60)), (S, chr3 + 700, F, 1, 0, eq(60)))
    add("ids of 254 bytes, no trim", (long_id, long_id), (r(), r()), (S, chr3 + 901, R, 1, 0, eq(60)), un)
    add("lower case and N, odd", (b"a5/1", b"a5/2"), ((b"acgtn" * 11, b"I" * 55), (b"nNacgtR" * 9, b"5" * 63)),
        (S, chr3 + 40, R, 10, 0, eq(55)), (S, chr3 + 240, F, 10, 0, eq(63)))
    n0, n = base.n, base.n + len(cases)
    results = pair_results(n)
    results[:n0] = base.results
    ends = ([], [])
    ids = [x.ids() for x in base.reads]
    for e in range(2):
        rd = base.reads[e]._p.contents
        for q in range(n0):
            front = int(base.clips[e][0][q])
            full = int(base.clips[e][1][q])
            start = rd.offsets[q] - front
            ends[e].append((ids[e][q], ctypes.string_at(rd.bases + start, full), ctypes.string_at(rd.quals + start, full)))
    ed = [int(v) for v in base.cigars.editDistance]
    ops = [[int(w) for w in base.cigars.ops[j, :base.cigars.nOps[j]]] for j in range(2 * n0)]
    for k, (_, cid, reads, recs) in enumerate(cases):
        q = n0 + k
        for e in range(2):
            st, loc, d, mq, dist, row = recs[e]
            results["status"][q, e], results["location"][q, e] = st, loc
            results["direction"][q, e], results["mapq"][q, e] = d, mq
            ed.append(dist)
            ops.append(row)
            ends[e].append((cid[e], reads[e][0], reads[e][1]))
    return PairBatch(ends, results, ed, ops), names + [c[0] for c in cases]


def unmapped_run_batch(n, first, last, seed=3, distinct=None):
    """n fabricated pairs on chr1, every end mapped with its own NM (7 + q % 50 for end 0, one more
    for end 1), except pairs [first, last) whose ends are both unmapped.  distinct: that many
    different locations per end, instead of one per pair (equal sort keys)."""
    rng = np.random.default_rng(seed)
    results = pair_results(n)
    ends = ([], [])
    ed, ops = [], []
    for q in range(n):
        gone = first <= q < last
        for e in range(2):
            b, ql = _read(rng, 40)
            ends[e].append((f"u{q}/{e + 1}".encode(), b, ql))
            if gone:
                results["status"][q, e] = snapgpu.NotFound
                ed.append(-1)
                ops.append([])
            else:
                results["status"][q, e] = snapgpu.SingleHit
                results["location"][q, e] = 500 + 3 * (q % distinct if distinct else q) + 200 * e
                results["direction"][q, e] = e
                results["mapq"][q, e] = 20
                ed.append(7 + q % 50 + e)
                ops.append([(40 << 4) | 7])
    return PairBatch(ends, results, ed, ops)


def python_sort_keys(index, records):
    """BAMFormat::getSortInfo (Bam.cpp:474-495) over decoded records, by piece index."""
    starts = piece_starts(index)
    keys = []
    for rec in records:
        f = record_fields(rec)
        if f["refID"] >= 0 and f["pos"] >= 0:
            keys.append(starts[f["refID"]] + f["pos"])
        elif f["next_refID"] >= 0 and f["next_pos"] >= 0:
            keys.append(starts[f["next_refID"]] + f["next_pos"])
        else:
            keys.append(0xFFFFFFFF)
    return np.array(keys, dtype=np.uint32)
