"""Helpers shared by test_bam_host.py (CPU) and test_bam_gpu.py: BAM record parsing, and small
made-up batches whose expected bytes always come from the host encoder (snapgpu.bam_format)."""
import struct

import numpy as np

import snapgpu

QUERY_OPS = (0, 1, 4, 7, 8)   # M I S = X consume query bases


def split_records(raw):
    """Concatenated BAM records -> list of bytes, each block_size + 4 long."""
    out, at = [], 0
    while at < len(raw):
        bs = struct.unpack_from("<i", raw, at)[0]
        assert bs >= 32 and at + 4 + bs <= len(raw), (at, bs, len(raw))
        out.append(raw[at:at + 4 + bs])
        at += 4 + bs
    return out


def fields(r):
    refID, pos, lrn, mapq, bin_, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", r, 4)
    o = 36
    name = r[o:o + lrn - 1]
    o += lrn
    ops = list(struct.unpack_from("<%dI" % ncig, r, o))
    o += 4 * ncig
    seq = r[o:o + (lseq + 1) // 2]
    o += (lseq + 1) // 2
    qual = r[o:o + lseq]
    aux = r[o + lseq:]
    assert aux[-7:-4] == b"NMi"
    return dict(name=name, refID=refID, pos=pos, mapq=mapq, bin=bin_, flag=flag, lseq=lseq, ops=ops, seq=seq, qual=qual,
                aux=aux, nm=struct.unpack("<i", aux[-4:])[0], nextRef=nref, nextPos=npos, tlen=tlen)


def made_up(locations, lengths, nm_values, directions=None, ids=None, n_ops=None, seed=11):
    """One read per entry: location 0xffffffff = NotFound (no CIGAR ops, NM carried), else a SingleHit
    with edit distance nm_values[i] and one "=" op (or n_ops[i] ops of 1 base each, the last taking
    the rest) -> (reads, ids, records, cigars)."""
    n = len(locations)
    rng = np.random.default_rng(seed)
    reads = snapgpu.Reads.from_list([("".join(rng.choice(list("ACGTNacgt"), size=int(l))),
                                      "".join(chr(c) for c in rng.integers(33, 74, size=int(l)))) for l in lengths])
    res = np.zeros(n, dtype=snapgpu.RESULT_DTYPE)
    res["location"] = np.asarray(locations, dtype=np.uint32)
    res["result"] = np.where(res["location"] == 0xFFFFFFFF, snapgpu.NotFound, snapgpu.SingleHit)
    res["direction"] = 0 if directions is None else np.asarray(directions, dtype=np.uint8)
    res["mapq"] = 30
    cig = snapgpu.Cigars.empty(n)
    for i in range(n):
        if res["location"][i] == 0xFFFFFFFF:
            continue
        cig.editDistance[i] = nm_values[i]
        k = 1 if n_ops is None else int(n_ops[i])
        cig.nOps[i] = k
        for j in range(k):
            count = 1 if j + 1 < k else max(0, int(lengths[i]) - (k - 1))
            cig.ops[i, j] = (count << 4) | (7 if j % 2 == 0 else 8)
    return reads, ([b"m%d" % i for i in range(n)] if ids is None else ids), res, cig


def permuted(raw, order):
    recs = split_records(raw)
    assert len(recs) == len(order)
    return b"".join(recs[int(i)] for i in order)
