"""Inputs shared by test_sam_line.py (CPU) and test_sam_gpu.py: the small-genome reads with the
reference's records and oracle CIGARs, and 5,000 fabricated records that reach every branch of the
SAM line (csrc/sam_line.h against samAppendLine, csrc/host/sam.cpp)."""
import ctypes as C
import os

import numpy as np

import snapgpu
from oracle_ffi import oracle_align, oracle_cigars

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

READ_LENGTHS = (0, 1, 2, 63, 64, 65, 500, 1024)
N_FABRICATED = 5000


def fastq(path):
    lines = open(path).read().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def small_index():
    return snapgpu.GenomeIndex.build(snapgpu.Genome.from_fasta(os.path.join(G, "small.fa"), 500), 20, 8)


def reference_results(n):
    """The reference's AlignRead records for the small reads (expected_small_default.tsv)."""
    res = np.zeros(n, dtype=snapgpu.RESULT_DTYPE)
    for i, l in enumerate(open(os.path.join(G, "expected_small_default.tsv")).read().splitlines()):
        x = l.split("\t")
        res[i]["result"], res[i]["location"], res[i]["direction"] = int(x[1]), int(x[2]), int(x[3])
        res[i]["score"], res[i]["mapq"] = int(x[4]), int(x[5])
    return res


def cigars_from_pairs(pairs):
    c = snapgpu.Cigars.empty(len(pairs))
    for i, (ed, s) in enumerate(pairs):
        c.editDistance[i] = ed
        k = 0
        num = ""
        for ch in s if ed >= 0 else "":
            if ch.isdigit():
                num += ch
            else:
                c.ops[i, k] = (int(num) << 4) | snapgpu.CIGAR_OPS.index(ch)
                k += 1
                num = ""
        c.nOps[i] = k
    return c


def small_case(idx, use_m):
    """(reads, ids, records, cigars, clip) of test_host_sam_format_matches_reference."""
    fq = fastq(os.path.join(G, "small_reads.fq"))
    reads = snapgpu.Reads.from_fastq(os.path.join(G, "small_reads.fq"))
    res = reference_results(len(fq))
    loc, dirs = snapgpu.cigar_inputs(res)
    cig = cigars_from_pairs(oracle_cigars(idx, [b for _, b, _ in fq], loc, dirs, use_m))
    return reads, [i for i, _, _ in fq], res, cig, None


def clipped_case(idx, use_m):
    """(reads, ids, records, cigars, clip) of test_clipped_sam_matches_reference_cpu."""
    fq = fastq(os.path.join(G, "small_reads.fq"))
    reads = snapgpu.Reads.from_fastq(os.path.join(G, "small_reads.fq"))
    clip = reads.clip(3)
    res = oracle_align(idx, reads, snapgpu.default_params())
    loc, dirs = snapgpu.cigar_inputs(res)
    cig = cigars_from_pairs(oracle_cigars(idx, [reads.get(i)[0] for i in range(reads.n)], loc, dirs, use_m))
    return reads, [i for i, _, _ in fq], res, cig, clip


def fabricated_case(idx, n=N_FABRICATED, seed=20261019):
    """n records over idx's genome that reach every branch of the line: result 0..3; location valid
    in every piece (the last included), 0xffffffff, 0 (before the first piece) and a piece's first
    base; both directions; mapq in [-5, 300]; ed in {-1, 0, 3, 31}; nOps in {0, 1, 64} with counts up
    to 2^28 - 1 and every op code; ids that are empty, hold a space at position 0, in the middle and at
    the end, and run to 200 bytes; read lengths 0, 1, 2, 63, 64, 65, 500, 1024; lower-case bases; a
    non-ACGTN byte, a 0x00 base and a 0x00 quality, each in forward and RC records."""
    rng = np.random.default_rng(seed)
    v = idx.view()
    piece = np.array(C.cast(v.pieceOffsets, C.POINTER(C.c_uint32))[:v.nPieces], dtype=np.int64)
    piece_end = np.append(piece[1:], v.nBases)
    lens = rng.choice(READ_LENGTHS, size=n, p=(.08, .08, .08, .16, .16, .24, .1, .1)).astype(np.uint32)
    lens[:len(READ_LENGTHS)] = READ_LENGTHS
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    total = int(lens.sum())
    bases = rng.choice(np.frombuffer(b"ACGTACGTACGTNacgtn", dtype=np.uint8), size=total)
    quals = rng.integers(33, 74, size=total, dtype=np.uint8)
    res = np.zeros(n, dtype=snapgpu.RESULT_DTYPE)
    res["result"] = rng.integers(0, 4, n)
    res["direction"] = rng.integers(0, 2, n)
    res["mapq"] = rng.integers(-5, 301, n)
    kind = rng.integers(0, 20, n)
    p = rng.integers(0, len(piece), n)
    p[:len(piece)] = np.arange(len(piece))          # every piece, the last included
    loc = piece[p] + (rng.random(n) * (piece_end[p] - piece[p])).astype(np.int64)
    loc = np.where(kind < 3, 0xFFFFFFFF, loc)        # no location
    loc = np.where(kind == 3, 0, loc)                # before the first piece
    loc = np.where(kind == 4, piece[p], loc)         # a piece's first base
    loc = np.where(kind == 5, piece_end[p] - 1, loc)  # its last
    loc[:len(piece)] = piece_end[:len(piece)] - 1 - np.arange(len(piece))
    res["location"] = loc.astype(np.uint32)
    # damage: one byte per chosen read, spread over forward and RC records by the draw above
    for what, buf, byte in (("base", bases, ord("X")), ("base", bases, 0x00), ("base", bases, 0xC3),
                            ("qual", quals, 0x00)):
        for i in np.nonzero((rng.random(n) < 0.08) & (lens > 0))[0]:
            buf[int(offs[i]) + int(rng.integers(0, lens[i]))] = byte
    cig = snapgpu.Cigars.empty(n)
    cig.editDistance[:] = rng.choice((-1, 0, 3, 31), size=n)
    cig.nOps[:] = rng.choice((0, 1, 64), size=n, p=(.2, .6, .2))
    counts = np.where(rng.random((n, 64)) < 0.5, rng.integers(0, 1 << 28, (n, 64)), rng.integers(0, 200, (n, 64)))
    counts[:, 0] = np.where(rng.random(n) < 0.1, (1 << 28) - 1, counts[:, 0])
    cig.ops[:, :] = (counts.astype(np.uint32) << 4) | rng.integers(0, 9, (n, 64)).astype(np.uint32)
    cig.ops[:9, 0] = (np.arange(1, 10, dtype=np.uint32) << 4) | np.arange(9, dtype=np.uint32)   # every op code
    ids = []
    for i in range(n):
        k = i % 7
        ids.append((b"", b" lead", b"mid dle/1", b"trailing ", b"q" * 200, b"x" * 99 + b" " + b"y" * 100,
                    b"r%d" % i)[k])
    reads = snapgpu.Reads.from_arrays(bases.tobytes(), quals.tobytes(), offs, lens)
    # the branches the docstring lists are in the draw
    mapped_rc = (res["result"] != 0) & (res["location"] != 0xFFFFFFFF) & (res["direction"] == 1)
    has = lambda buf, byte: np.array([byte in buf[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)])
    for buf, byte in ((bases, b"X"), (bases, b"\0"), (quals, b"\0")):
        h = has(buf, byte)
        assert (h & mapped_rc).any() and (h & ~mapped_rc).any()
    return reads, ids, res, cig, None


READ_GROUPS = (None, "", "FASTQ")
