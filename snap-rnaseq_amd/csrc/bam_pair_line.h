// bam_pair_line.h -- the two BAM records of a read pair without transcriptome CIGAR, as the paired
// writer appends them (host/rna_paired.cpp's record loop over bamAppendRecord with SamLine::hasMate,
// host/bam.cpp; BAMFormat::writeRead with a mate, Bam.cpp:596-790), restated over plain pointers for
// host and device: the exact size of record j (block_size + 4), and a writer that stores exactly
// those bytes.
//
// Built over sam_pair_line.h, which says once which end record j is, its flags, where it and its
// mate lie and TLEN (pairPlace, pairExtents, pairIdLen; the same PairArgs and CIGAR row strides), and
// over bam_line.h for the record layout (codes, bin, SEQ / QUAL packing, tags).  Both parts are
// templates over their group G.
//
// Where the record differs from the SAM line of the same end: the QNAME is the whole id after the
// "/1" "/2" trim, not cut at the first space; refID and next_refID are piece indices (no "=");
// tlen is truncated to 32 bits; SEQ and QUAL cover the whole unclipped read; an end with a location
// writes its own edit distance as NM, even -1, and an end without one repeats the NM of the record
// written before it (nmOwn below is kNoNm for it: the caller resolves it in write order).
#pragma once
#include "bam_line.h"
#include "sam_pair_line.h"

namespace bampairline {

using samline::kInvalid;
using samline::PairArgs;

// "no NM of its own".  Not -1 as in bam_line.h: a mapped end without CIGAR carries -1 on.
constexpr int32_t kNoNm = INT32_MIN;

// What fields() decides about one record; write() places bytes by it.
struct Fields {
    uint64_t readStart;   // first byte of the unclipped read in bases / quals of `end`
    uint32_t end;         // the end this record holds
    uint32_t qlen;        // QNAME: the trimmed id
    uint32_t flags, mapq, bin;
    int32_t refID, pos;           // piece index and 0-based position; the mate's for an unmapped end
    int32_t nextRef, nextPos;     // the mate's; the record's own where the mate is unmapped
    int32_t tlen;
    uint32_t before, after, nOps, nCigar;
    uint32_t len, rc;     // l_seq: the unclipped length
    int32_t nmOwn;        // the record's own NM, or kNoNm
};

// refID, pos, next_refID, next_pos, FLAG and MAPQ of record j, from the pair record and the piece
// offsets alone -> where the two ends lie (snapgpu_bam_pair_sort_keys reads no more).
SAM_HD samline::PairPlace place(const PairArgs &A, uint64_t j, samline::PairFields &P, Fields &F) {
    const samline::PairPlace L = samline::pairPlace(A, j, P);
    F.end = P.end;
    F.flags = P.F.flags;
    F.mapq = P.F.mapq;
    F.rc = P.F.rc;
    F.refID = P.F.piece;
    F.pos = (int32_t)(P.F.pos - 1u);
    F.nextRef = samline::pairMateIndex(P);
    F.nextPos = (int32_t)(P.pnext - 1u);
    return L;
}

// The coordinate-sort key of the record F describes: BAMFormat::getSortInfo (Bam.cpp:474-495) -- the
// record's own place when it has one, else its mate's, else UINT32_MAX.  By piece index.
SAM_HD uint32_t sortKey(const PairArgs &A, const Fields &F) {
    if (F.refID >= 0 && F.pos >= 0) return A.pieceOffsets[F.refID] + (uint32_t)F.pos;
    if (F.nextRef >= 0 && F.nextPos >= 0) return A.pieceOffsets[F.nextRef] + (uint32_t)F.nextPos;
    return kInvalid;
}

template <class G>
SAM_HD Fields fields(const PairArgs &A, uint64_t j, const G &g) {
    Fields F;
    samline::PairFields P;
    const samline::PairPlace L = place(A, j, P, F);
    samline::pairExtents(A, j, L, P);
    const uint64_t q = j >> 1;
    F.readStart = P.F.readStart;
    F.len = P.F.fullLen;
    F.before = P.F.before;
    F.after = P.F.after;
    F.tlen = (int32_t)P.tlen;
    F.qlen = samline::pairIdLen(A, q, F.end);
    // CIGAR ops only at a location with an edit distance; NM at every location
    const uint64_t row = q * A.rowPair + F.end * A.rowEnd;
    const bool own = L.loc != kInvalid;
    F.nmOwn = own ? A.ed[row] : kNoNm;
    const bool cigar = own && A.ed[row] >= 0;
    F.nOps = A.nOps[row] < SNAPGPU_CIGAR_MAX_OPS ? A.nOps[row] : SNAPGPU_CIGAR_MAX_OPS;   // a row holds no more
    F.nCigar = cigar ? (F.before ? 1u : 0u) + F.nOps + (F.after ? 1u : 0u) : 0u;
    // the reference span: the ops' (soft clips consume none), the read's length without ops; the
    // sum wraps as the reference's int does
    uint32_t refLength = F.len;
    if (F.nCigar) {
        const uint32_t *ops = A.ops + row * SNAPGPU_CIGAR_MAX_OPS;
        refLength = g.sum(F.nOps, [=](uint32_t k) { return bamline::refBase(ops[k]) * (ops[k] >> 4); });
    }
    // unmapped: one base at the mate's position, or at -1 (Bam.cpp:752-756)
    F.bin = (uint32_t)(own                     ? bamline::reg2bin(F.pos, (int32_t)((uint32_t)F.pos + refLength))
                       : L.mateLoc != kInvalid ? bamline::reg2bin(F.nextPos, (int32_t)((uint32_t)F.nextPos + 1u))
                                               : bamline::reg2bin(-1, 0));
    return F;
}

// block_size + 4
SAM_HD uint32_t recordLength(const PairArgs &A, const Fields &F) {
    return 36 + F.qlen + 1 + 4 * F.nCigar + (F.len + 1) / 2 + F.len + bamline::tagsLength(A.rg, A.rgLen);
}

// The bytes of record j at output offset `at`: exactly recordLength(A, F) of them.  nm: the NM value
// (F.nmOwn, or the carried one where that is kNoNm).
template <class G>
SAM_HD void write(const PairArgs &A, uint64_t j, const Fields &F, int32_t nm, uint64_t at, const G &g) {
    using bamline::put16;
    using bamline::put32;
    const uint64_t q = j >> 1;
    const uint32_t e = F.end;
    uint64_t p = at + 36 + F.qlen + 1;
    if (g.lead()) {
        put32(g, at, recordLength(A, F) - 4);   // block_size
        put32(g, at + 4, (uint32_t)F.refID);
        put32(g, at + 8, (uint32_t)F.pos);
        g.put(at + 12, (char)(F.qlen + 1));     // l_read_name
        g.put(at + 13, (char)F.mapq);
        put16(g, at + 14, F.bin & 0xffff);
        put16(g, at + 16, F.nCigar);
        put16(g, at + 18, F.flags);
        put32(g, at + 20, F.len);               // l_seq
        put32(g, at + 24, (uint32_t)F.nextRef);
        put32(g, at + 28, (uint32_t)F.nextPos);
        put32(g, at + 32, (uint32_t)F.tlen);
        g.put(at + 36 + F.qlen, '\0');
        // soft clips around the ops, mirrored for RC
        uint64_t w = p;
        if (F.nCigar) {
            const uint32_t *ops = A.ops + (q * A.rowPair + e * A.rowEnd) * SNAPGPU_CIGAR_MAX_OPS;
            if (F.before) { put32(g, w, F.before << 4 | 4u); w += 4; }
            for (uint32_t k = 0; k < F.nOps; k++) { put32(g, w, ops[k]); w += 4; }
            if (F.after) put32(g, w, F.after << 4 | 4u);
        }
    }
    const char *id = A.ids[e] + A.idOffsets[e][q];
    g.copy(at + 36, F.qlen, [=](uint32_t k) { return id[k]; });
    p += 4 * F.nCigar;
    bamline::seqQual(A.bases[e] + F.readStart, A.quals[e] + F.readStart, F.len, F.rc, p, g);
    p += (F.len + 1) / 2 + F.len;
    bamline::tags(A.rg, A.rgLen, nm, p, g);
}

using samline::Serial;

}  // namespace bampairline
