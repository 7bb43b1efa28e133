"""Shared inputs of the paired SAM formatter tests (test_sam_pairs_host.py, test_sam_pairs_gpu.py).

decode_fixture(): the reference's own paired SAM records (expected_rna_paired.sam.gz,
expected_rna150_paired.sam.gz, written on the index of small.fa) decoded back into the formatter's
inputs -- ids, reads, clip state, pair records and CIGAR rows -- so that the formatter can be held
to the reference's bytes without an aligner.  fabricated(): small hand-made pair batches for the
branches no fixture of the reference reaches.  python_lines(): the mate rule in plain Python."""
import ctypes
import functools
import gzip
import os

import numpy as np

import snapgpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = "MIDNSHP=X"
INVALID = 0xFFFFFFFF
FIXTURES = {"rna": 2999, "rna150": 2000}   # stem -> pairs
_COMP = bytes.maketrans(b"ACGTNn", b"TGCANn")


@functools.lru_cache(maxsize=None)
def small_index():
    """The index of tests/golden/small.fa (chr1..chr3) the fixtures were written on."""
    return snapgpu.GenomeIndex.build(snapgpu.Genome.from_fasta(os.path.join(G, "small.fa"), 500), 20, 4)


def piece_offsets(index):
    """name -> first location, from the index's genome."""
    return {(n.decode() if isinstance(n, bytes) else n): int(o) for n, o in index_pieces(index)}


def index_pieces(index):
    g = snapgpu.Genome(index.genome_handle())
    try:
        return list(g.pieces)
    finally:
        g._h = None   # the index owns the genome


def revcomp(b):
    return b.translate(_COMP)[::-1]


def parse_cigar(text):
    """-> (soft clip before, op rows as count << 4 | code, soft clip after)."""
    tok, num = [], 0
    for ch in text:
        if ch.isdigit():
            num = num * 10 + int(ch)
        else:
            tok.append((num, ch))
            num = 0
    before = after = 0
    if tok and tok[0][1] == "S":
        before = tok.pop(0)[0]
    if tok and tok[-1][1] == "S":
        after = tok.pop()[0]
    assert all(c != "S" for _, c in tok)
    return before, [(n << 4) | OPS.index(c) for n, c in tok], after


class PairBatch:
    """Formatter inputs of n pairs: reads0 / reads1 (with ids and clip state), results, cigars."""

    def __init__(self, ends, results, ed, ops, clipping=3):
        """ends: [end][pair] -> (id bytes, bases, quals); ops: 2n lists of op words."""
        n = len(results)
        self.n = n
        self.reads = []
        self.clips = []
        for e in range(2):
            fq = b"".join(b"@" + i + b"\n" + b + b"\n+\n" + q + b"\n" for i, b, q in ends[e])
            r = snapgpu.Reads.from_fastq_bytes(fq)
            assert r.n == n
            self.clips.append(r.clip(clipping) if clipping is not None else None)
            self.reads.append(r)
        self.results = np.ascontiguousarray(results, dtype=snapgpu.PAIR_RESULT_DTYPE)
        c = snapgpu.Cigars.empty(2 * n)
        c.editDistance[:] = ed
        for r, row in enumerate(ops):
            c.nOps[r] = len(row)
            c.ops[r, :len(row)] = row
        self.cigars = c

    def args(self):
        return self.reads[0], self.reads[1], self.results, self.cigars

    def exchanged(self):
        """The same pairs with end 0 and end 1 swapped."""
        x = object.__new__(PairBatch)
        x.n = self.n
        x.reads = self.reads[::-1]
        x.clips = self.clips[::-1]
        x.results = self.results.copy()
        for f in ("location", "score", "mapq", "status", "direction"):
            x.results[f] = self.results[f][:, ::-1]
        c = snapgpu.Cigars.empty(2 * self.n)
        for a in ("editDistance", "nOps", "ops"):
            src = getattr(self.cigars, a)
            dst = getattr(c, a)
            dst[0::2], dst[1::2] = src[1::2], src[0::2]
        x.cigars = c
        return x


def pair_results(n):
    r = np.zeros(n, dtype=snapgpu.PAIR_RESULT_DTYPE)
    r["location"] = INVALID
    r["score"] = -1
    return r


@functools.lru_cache(maxsize=None)
def decode_fixture(stem, suffix_ids=False):
    """-> (PairBatch, [line bytes] of the 2n records, counts dict).  The first line of a pair is taken
    as end 0: it is the end at the lower (or equal) location, which the rule writes first.
    suffix_ids: give the ids back the "/1" and "/2" the writer dropped."""
    index = small_index()
    off = piece_offsets(index)
    raw = gzip.open(os.path.join(G, f"expected_{stem}_paired.sam.gz"), "rb").read().split(b"\n")
    lines = [l + b"\n" for l in raw if l and not l.startswith(b"@")]
    n = len(lines) // 2
    assert len(lines) == 2 * n
    results = pair_results(n)
    ends = ([], [])
    ed, ops, want_clip = [], [], []
    counts = dict(other_piece=0, soft_clipped_pairs=0, n_ops=0, max_ops=0, flags=set())
    for j, line in enumerate(lines):
        q, e = divmod(j, 2)
        f = line[:-1].decode().split("\t")
        assert len(f) == 14 and f[11] == "RG:Z:FASTQ" and f[12] == "PG:Z:SNAP" and f[13].startswith("NM:i:")
        flag = int(f[1])
        counts["flags"].add(flag)
        seq, qual = f[9].encode(), f[10].encode()
        assert len(seq) == len(qual)
        rc = bool(flag & 0x10)
        mapped = not flag & 0x4
        before = after = 0
        row = []
        if mapped:
            assert f[5] != "*"
            before, row, after = parse_cigar(f[5])
            results["status"][q, e] = snapgpu.SingleHit if int(f[4]) > 10 else snapgpu.MultipleHits
            results["location"][q, e] = off[f[2]] + int(f[3]) - 1
            results["direction"][q, e] = int(rc)
            results["mapq"][q, e] = int(f[4])
            counts["max_ops"] = max(counts["max_ops"], len(row))
            counts["n_ops"] += any((w & 15) == 3 for w in row)
            counts["other_piece"] += f[6] not in ("=", "*")
        else:
            assert not rc and f[5] == "*"
        front, back = (after, before) if rc else (before, after)
        want_clip.append((mapped, front, len(seq)))
        ed.append(int(f[13][5:]))
        ops.append(row)
        name = f[0].encode() + ((b"/1", b"/2")[e] if suffix_ids else b"")
        ends[e].append((name, revcomp(seq) if rc else seq, qual[::-1] if rc else qual))
    batch = PairBatch(ends, results, ed, ops)
    # Read::clip of the decoded qualities gives back the soft clips the reference printed
    clipped_pairs, clipped_first = set(), set()
    for j, (mapped, front, full) in enumerate(want_clip):
        q, e = divmod(j, 2)
        got_front, got_full = batch.clips[e][0][q], batch.clips[e][1][q]
        assert got_full == full
        if mapped:
            assert got_front == front, (stem, j)
            row_len = sum(w >> 4 for w in ops[j] if (w & 15) in (0, 1, 7, 8))
            if row_len != full:
                clipped_pairs.add(q)
                if e == 0:
                    clipped_first.add(q)
            assert batch.reads[e].lengths()[q] == row_len, (stem, j)
    counts["soft_clipped_pairs"] = len(clipped_pairs)
    counts["soft_clipped_first"] = len(clipped_first)
    return batch, lines, counts


def split_lines(text):
    return text.splitlines(keepends=True)


def python_lines(index, batch, read_group="FASTQ"):
    """The 2n lines by a plain restatement of the rule (which end first, flags, RNEXT / PNEXT / POS of
    mapped, half-mapped and unmapped pairs, TLEN from the clipped extents)."""
    pieces = [(n.decode() if isinstance(n, bytes) else n, int(o)) for n, o in index_pieces(index)]

    def piece(loc):
        best = None
        for name, o in pieces:
            if o <= loc:
                best = (name, o)
        return best

    out = []
    res = batch.results
    ids = [r.ids() for r in batch.reads]
    lens = [r.lengths() for r in batch.reads]
    for q in range(batch.n):
        locs = [int(res["location"][q, e]) if res["status"][q, e] != snapgpu.NotFound else INVALID for e in range(2)]
        first = int(locs[0] > locs[1])
        i0, i1 = ids[0][q], ids[1][q]
        trim = 0
        if len(i0) == len(i1) and len(i0) > 2 and i0[-2:-1] == b"/" and i1[-2:-1] == b"/":
            c0, c1 = i0[-1:], i1[-1:]
            if c0 in (b"1", b"2") and (c0 == b"1" or c1 == b"2") and c0 != c1:
                trim = 2
        ext = []
        for e in range(2):
            front = int(batch.clips[e][0][q]) if batch.clips[e] is not None else 0
            clipped = int(lens[e][q])
            full = int(batch.clips[e][1][q]) if batch.clips[e] is not None else clipped
            ext.append((front, clipped, full))
        for w in range(2):
            e = first if w == 0 else 1 - first
            m = 1 - e
            loc, mloc = locs[e], locs[m]
            front, clipped, full = ext[e]
            back = full - clipped - front
            rc = loc != INVALID and res["direction"][q, e] == snapgpu.RC
            flags = 0x1 | (0x40 if w == 0 else 0x80)
            rname, pos, mapq = "*", 0, 0
            if loc != INVALID:
                flags |= 0x10 if rc else 0
                rname, o = piece(loc)
                pos = loc - o + 1
                mapq = max(0, min(70, int(res["mapq"][q, e])))
            else:
                flags |= 0x4
            rnext, pnext, tlen = "*", 0, 0
            if mloc != INVALID:
                mname, mo = piece(mloc)
                rnext, pnext = mname, mloc - mo + 1
                if res["direction"][q, m] == snapgpu.RC:
                    flags |= 0x20
                if loc == INVALID:
                    rname, pos, rnext = mname, pnext, "="
            else:
                flags |= 0x8
                rnext, pnext = "=", pos
            before, after = (back, front) if rc else (front, back)
            if loc != INVALID and mloc != INVALID:
                flags |= 0x2
                if rname == rnext:
                    rnext = "="
                    mfront, mclipped, mfull = ext[m]
                    mback = mfull - mclipped - mfront
                    mrc = res["direction"][q, m] == snapgpu.RC
                    my_start, my_end = loc - before, loc + clipped + after
                    mate_start = mloc - (mback if mrc else mfront)
                    mate_end = mloc + mclipped + (mfront if mrc else mback)
                    tlen = mate_end - my_start if my_start < mate_start else -(my_end - mate_start)
            row = 2 * q + e
            ed = int(batch.cigars.editDistance[row]) if loc != INVALID else -1
            cigar = "*"
            if loc != INVALID and ed >= 0:
                cigar = (f"{before}S" if before else "") + batch.cigars.string(row) + (f"{after}S" if after else "")
            b, ql = batch.reads[e].get(q)   # the clipped read; the unclipped one around it
            r = batch.reads[e]._p.contents
            start = r.offsets[q] - front
            b = ctypes.string_at(r.bases + start, full)
            ql = ctypes.string_at(r.quals + start, full)
            if rc:   # a base without complement ends SEQ (it prints as NUL)
                b, ql = b.upper()[::-1], ql[::-1]
                stop = next((k for k, c in enumerate(b) if c not in b"ACGTN"), len(b))
                b = b[:stop].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))
            else:
                b = b.upper()
            name = ids[e][q][:len(ids[e][q]) - trim].split(b" ")[0].decode()
            tags = ([] if read_group is None else [f"RG:Z:{read_group}"]) + ["PG:Z:SNAP", f"NM:i:{ed}"]
            out.append("\t".join([name, str(flags), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen),
                                  b.decode(), ql.decode()] + tags).encode() + b"\n")
    return out


def _read(rng, n, front=0, back=0):
    """(bases, quals) of n bases whose first `front` and last `back` qualities are '#' (Read::clip)."""
    b = bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    return b, b"#" * front + b"I" * (n - front - back) + b"#" * back


@functools.lru_cache(maxsize=None)
def fabricated():
    """-> (PairBatch, [case name per pair]): the branches the reference's fixtures do not reach, on
    the pieces of small.fa (chr1 at 500, chr2 at 117293, chr3 at 230679)."""
    rng = np.random.default_rng(22)
    chr1, chr2, chr3 = 500, 117293, 230679
    S, M, NF, F, R = snapgpu.SingleHit, snapgpu.MultipleHits, snapgpu.NotFound, snapgpu.FORWARD, snapgpu.RC
    eq = lambda n: [(n << 4) | 7]
    cases = []   # name, (id0, id1), (read0, read1), per end (status, location, direction, mapq, ed, ops)

    def add(name, ids, reads, e0, e1):
        cases.append((name, ids, reads, (e0, e1)))

    r = lambda n=60, f=0, b=0: _read(rng, n, f, b)
    add("half mapped, end 0", (b"h0/1", b"h0/2"), (r(), r()), (S, chr1 + 100, F, 60, 1, eq(60)), (NF, INVALID, F, 0, -1, []))
    add("half mapped, end 1 RC", (b"h1/1", b"h1/2"), (r(), r()), (NF, INVALID, R, 0, -1, []), (S, chr2 + 7, R, 33, 0, eq(60)))
    add("half mapped, stale location", (b"h2/1", b"h2/2"), (r(), r()), (NF, chr1 + 5, R, 9, 3, eq(60)), (M, chr3 + 1, F, 3, 2, eq(60)))
    add("both unmapped", (b"u/1", b"u/2"), (r(), r()), (NF, INVALID, F, 0, -1, []), (NF, INVALID, R, 0, -1, []))
    add("equal locations", (b"e/1", b"e/2"), (r(), r()), (S, chr1 + 4000, F, 70, 0, eq(60)), (S, chr1 + 4000, R, 70, 0, eq(60)))
    add("end 1 lower", (b"l/1", b"l/2"), (r(), r()), (S, chr1 + 9000, R, 50, 2, eq(60)), (S, chr1 + 8800, F, 51, 1, eq(60)))
    add("different pieces", (b"d/1", b"d/2"), (r(), r()), (S, chr1 + 10, F, 20, 0, eq(60)), (M, chr3 + 70000, R, 5, 4, eq(60)))
    add("negative and long TLEN", (b"t/1", b"t/2"), (r(), r()), (S, chr1 + 116000, R, 70, 0, eq(60)), (S, chr1, F, 70, 0, eq(60)))
    add("different clips", (b"c/1", b"c/2"), (r(70, 3, 0), r(66, 2, 5)),
        (S, chr2 + 500, F, 44, 1, [(30 << 4) | 7, (1 << 4) | 8, (36 << 4) | 7]),
        (S, chr2 + 700, R, 45, 2, [(20 << 4) | 7, (2 << 4) | 1, (37 << 4) | 7]))
    add("different clips, both RC", (b"k/1", b"k/2"), (r(70, 4, 6), r(64, 0, 9)),
        (S, chr2 + 900, R, 44, 0, eq(60)), (S, chr2 + 650, R, 45, 0, eq(55)))
    add("MAPQ above 70 and below 0", (b"m/1", b"m/2"), (r(), r()), (S, chr3 + 5, F, 99, 0, eq(60)), (M, chr3 + 300, R, -4, 0, eq(60)))
    add("ids /2 /1", (b"x/2", b"x/1"), (r(), r()), (S, chr1 + 20, F, 1, 0, eq(60)), (S, chr1 + 300, R, 1, 0, eq(60)))
    add("ids /1 /1", (b"y/1", b"y/1"), (r(), r()), (S, chr1 + 21, F, 1, 0, eq(60)), (S, chr1 + 301, R, 1, 0, eq(60)))
    add("ids /2 /2", (b"w/2", b"w/2"), (r(), r()), (S, chr1 + 21, F, 1, 0, eq(60)), (S, chr1 + 301, R, 1, 0, eq(60)))
    add("ids /3 /2", (b"v/3", b"v/2"), (r(), r()), (S, chr1 + 21, F, 1, 0, eq(60)), (S, chr1 + 301, R, 1, 0, eq(60)))
    add("ids of unequal length", (b"long-name/1", b"nm/2"), (r(), r()), (S, chr1 + 22, F, 1, 0, eq(60)), (S, chr1 + 302, R, 1, 0, eq(60)))
    add("space before the suffix", (b"sp ace/1", b"sp ace/2"), (r(), r()), (S, chr1 + 23, F, 1, 0, eq(60)), (S, chr1 + 303, R, 1, 0, eq(60)))
    add("suffix only", (b"/1", b"/2"), (r(), r()), (S, chr1 + 24, F, 1, 0, eq(60)), (S, chr1 + 304, R, 1, 0, eq(60)))
    nul = r()
    nul = (nul[0][:40] + b"R" + nul[0][41:], nul[1])   # COMPLEMENT['R'] is 0: SEQ of the RC end stops there
    add("a base that complements to NUL", (b"n/1", b"n/2"), (r(), nul), (S, chr2 + 30, F, 10, 0, eq(60)), (S, chr2 + 230, R, 10, 1, eq(60)))
    add("mapped without CIGAR", (b"z/1", b"z/2"), (r(), r()), (S, chr2 + 31, F, 10, -1, []), (S, chr2 + 231, R, 10, 0, eq(60)))
    add("a full row of ops", (b"f/1", b"f/2"), (r(64), r(64)), (S, chr2 + 32, F, 10, 30, [(1 << 4) | (7 + (k & 1)) for k in range(64)]),
        (S, chr2 + 232, R, 10, 0, eq(64)))
    add("lower case and N", (b"a/1", b"a/2"), ((b"acgtn" * 12, b"I" * 60), (b"acgtN" * 12, b"I" * 60)),
        (S, chr3 + 40, F, 10, 0, eq(60)), (S, chr3 + 240, R, 10, 0, eq(60)))
    n = len(cases)
    results = pair_results(n)
    ends = ([], [])
    ed, ops = [], []
    for q, (_, ids, reads, recs) in enumerate(cases):
        for e in range(2):
            st, loc, d, mq, k, row = recs[e]
            results["status"][q, e], results["location"][q, e] = st, loc
            results["direction"][q, e], results["mapq"][q, e] = d, mq
            ed.append(k)
            ops.append(row)
            ends[e].append((ids[e], reads[e][0], reads[e][1]))
    return PairBatch(ends, results, ed, ops), [c[0] for c in cases]


def too_long_batch():
    """One pair whose end 1 has 1,025 bases: past the formatter's SEQ / QUAL limit."""
    rng = np.random.default_rng(5)
    a, b = _read(rng, 60), _read(rng, 1025)
    res = pair_results(1)
    return PairBatch(([(b"p/1", a[0], a[1])], [(b"p/2", b[0], b[1])]), res, [-1, -1], [[], []])


def synthetic_batch(genome, n, clipped, seed=31, read_length=101, id_length=0):
    """(reads0, reads1) of n wgsim-like pairs on `genome` with ids "r<i>/1" "r<i>/2" (padded to
    id_length).  clipped: about half the reads get '#' quality tails, then Read::clip(3); about one
    end in seven is replaced by random bases, so that half-mapped and unmapped pairs occur."""
    src = snapgpu.Reads.synthetic_pairs(genome, n, seed=seed, read_length=read_length,
                                        insert_mean=max(300, 2 * read_length + 100), insert_sd=30)
    rng = np.random.default_rng(seed)
    out = []
    for e in range(2):
        fq = []
        for i in range(n):
            b, q = src[e].get(i)
            if clipped:
                if rng.random() < 0.5:
                    f, k = int(rng.integers(0, 5)), int(rng.integers(0, 7))
                    q = b"#" * f + q[f:len(q) - k] + b"#" * k
                if rng.random() < 0.15:
                    b = bytes(rng.choice(list(b"ACGT"), len(b)).astype(np.uint8))
            name = f"r{i}".encode()
            name += b"x" * max(0, id_length - len(name) - 2) + (b"/1", b"/2")[e]
            fq.append(b"@" + name + b"\n" + b + b"\n+\n" + q + b"\n")
        r = snapgpu.Reads.from_fastq_bytes(b"".join(fq))
        if clipped:
            r.clip(3)
        out.append(r)
    return out[0], out[1]
