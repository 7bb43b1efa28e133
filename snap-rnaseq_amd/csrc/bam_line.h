// bam_line.h -- one BAM record of a read without mate and without transcriptome CIGAR, as
// bamAppendRecord (host/bam.cpp) appends it, restated over plain pointers for host and device:
// the exact size of record i (block_size + 4), and a writer that stores exactly those bytes.
//
// The inputs are sam_line.h's Args and both parts are templates over its "group" G (firstOf is not
// used).  Serial is one host thread (snapgpu_bam_format); bam_format.hip has the 64-lane wave that
// writes into an LDS window.  Every member of a group calls fields() / write() with the same arguments.
//
// Kept from the reference (BAMFormat::writeRead, Bam.cpp:596-790): the QNAME is the whole id; SEQ and
// QUAL cover the whole unclipped read; the record's own location decides CIGAR, bin and NM even for a
// NotFound record, while refID, pos, FLAG and MAPQ take NotFound as unmapped; a record without CIGAR
// ops carries the NM of the record before it (nmOwn below is kNoNm for it: the caller resolves it).
#pragma once
#include "sam_line.h"

namespace bamline {

using samline::Args;
using samline::kInvalid;

constexpr uint32_t kMaxQname = 254;   // l_read_name is one byte and counts the NUL (Bam.cpp:723-726)
constexpr int32_t kNoNm = -1;         // "no NM of its own": an edit distance is never negative

// What fields() decides about one record; write() places bytes by it.
struct Fields {
    uint64_t readStart;   // first byte of the unclipped read in bases / quals
    uint32_t qlen;        // QNAME: the whole id
    uint32_t flags, mapq, bin;
    int32_t refID, pos;   // piece index and 0-based position, -1 and -1 without a piece
    uint32_t cigar;       // 1: soft clips + ops; 0: no ops
    uint32_t before, after, nOps, nCigar;
    uint32_t len, rc;     // l_seq: the unclipped length
    int32_t nmOwn;        // the record's own NM, or kNoNm
};

// BAMAlignment::SeqToCode from CodeToSeq = "=ACMGRSVTWYHKDBN" (Bam.cpp:179, :266-276); '=' and
// every byte that is not in the string give 0
SAM_HD uint32_t seqCode(char c) {
    switch (c) {
        case 'A': return 1;
        case 'C': return 2;
        case 'M': return 3;
        case 'G': return 4;
        case 'R': return 5;
        case 'S': return 6;
        case 'V': return 7;
        case 'T': return 8;
        case 'W': return 9;
        case 'Y': return 10;
        case 'H': return 11;
        case 'K': return 12;
        case 'D': return 13;
        case 'B': return 14;
        case 'N': return 15;
        default: return 0;
    }
}

// CigarCodeToRefBase (Bam.cpp:183): M, D, N, P, = and X consume reference bases
SAM_HD uint32_t refBase(uint32_t op) { return (0x1cdu >> (op & 15u)) & 1u; }

// BAMAlignment::reg2bin (Bam.cpp:279-291); beg may be -1 (arithmetic shifts, as the reference's ints)
SAM_HD int32_t reg2bin(int32_t beg, int32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
    return 0;
}

// refID and pos of record i alone (F.refID, F.pos) -> the location they come from: NotFound ->
// unmapped (kInvalid).  Reads A.res and the piece offsets only (snapgpu_bam_sort_keys).
SAM_HD uint32_t locate(const Args &A, uint64_t i, Fields &F) {
    uint32_t loc = A.res[i].location;
    if (A.res[i].result == SNAPGPU_NOT_FOUND) loc = kInvalid;
    F.refID = -1;
    F.pos = -1;
    if (loc != kInvalid) {
        const int32_t p = samline::pieceAt(A.pieceOffsets, A.nPieces, loc);
        if (p >= 0) {
            F.refID = p;
            F.pos = (int32_t)(loc - A.pieceOffsets[p]);
        }
    }
    return loc;
}

// The coordinate-sort key of the record F describes: BAMFormat::getSortInfo (Bam.cpp:474-495) for a
// read without mate -- the record's genome location when it has a refID, else UINT32_MAX.  By piece
// index: two pieces of one name keep their own offsets (samline::sortKey goes by the first of the name).
SAM_HD uint32_t sortKey(const Args &A, const Fields &F) {
    return F.refID < 0 ? kInvalid : A.pieceOffsets[F.refID] + (uint32_t)F.pos;
}

template <class G>
SAM_HD Fields fields(const Args &A, uint64_t i, const G &g) {
    Fields F;
    const uint32_t front = A.front ? A.front[i] : 0u;
    const uint32_t clipped = A.lengths[i];
    F.len = A.unclipped ? A.unclipped[i] : clipped;
    F.readStart = A.offsets[i] - front;
    const uint32_t recLoc = A.res[i].location;
    const uint32_t loc = locate(A, i, F);
    F.rc = loc != kInvalid && A.res[i].direction == SNAPGPU_RC;
    F.flags = 0;
    F.mapq = 0;
    if (loc != kInvalid) {
        if (F.rc) F.flags |= 0x10;   // SAM_REVERSE_COMPLEMENT
        int32_t m = A.res[i].mapq;
        m = m > 70 ? 70 : m;
        F.mapq = (uint32_t)(m < 0 ? 0 : m);
    } else {
        F.flags |= 0x04;             // SAM_UNMAPPED
    }
    F.qlen = A.idLengths[i];
    // CIGAR ops and NM at writeRead's own location, even for NotFound (Bam.cpp:654-679)
    F.cigar = recLoc != kInvalid && A.ed[i] >= 0;
    F.nmOwn = F.cigar ? A.ed[i] : kNoNm;
    const uint32_t back = F.len - clipped - front;
    F.before = F.rc ? back : front;
    F.after = F.rc ? front : back;
    F.nOps = A.nOps[i] < SNAPGPU_CIGAR_MAX_OPS ? A.nOps[i] : SNAPGPU_CIGAR_MAX_OPS;   // a row holds no more
    F.nCigar = F.cigar ? (F.before ? 1u : 0u) + F.nOps + (F.after ? 1u : 0u) : 0u;
    // the reference span: the ops' (soft clips consume none), the read's length without ops; the
    // sum wraps as the reference's int does
    uint32_t refLength = F.len;
    if (F.nCigar) {
        const uint32_t *ops = A.ops + i * SNAPGPU_CIGAR_MAX_OPS;
        refLength = g.sum(F.nOps, [=](uint32_t k) { return refBase(ops[k]) * (ops[k] >> 4); });
    }
    // unmapped without mate: at -1, length 1 (Bam.cpp:752-756)
    F.bin = (uint32_t)(recLoc != kInvalid ? reg2bin(F.pos, (int32_t)((uint32_t)F.pos + refLength)) : reg2bin(-1, 0));
    return F;
}

// the tags after QUAL: RG:Z (with a read group), PG:Z:SNAP, NM:i
SAM_HD uint32_t tagsLength(const char *rg, uint32_t rgLen) { return (rg ? 4 + rgLen : 0) + 8 + 7; }
SAM_HD uint32_t tagsLength(const Args &A) { return tagsLength(A.rg, A.rgLen); }

// block_size + 4
SAM_HD uint32_t recordLength(const Args &A, const Fields &F) {
    return 36 + F.qlen + 1 + 4 * F.nCigar + (F.len + 1) / 2 + F.len + tagsLength(A);
}

template <class G>
SAM_HD void put16(const G &g, uint64_t at, uint32_t v) {
    g.put(at, (char)(v & 0xff));
    g.put(at + 1, (char)((v >> 8) & 0xff));
}
template <class G>
SAM_HD void put32(const G &g, uint64_t at, uint32_t v) {
    put16(g, at, v & 0xffff);
    put16(g, at + 2, v >> 16);
}

// SEQ and QUAL of the whole unclipped read B / Q of len bases at p, reverse-complemented / reversed
// for RC.  SEQ: byte k holds bases 2k (high nibble) and 2k + 1; an odd tail has a zero low nibble.
// QUAL: phred values.  (len + 1) / 2 + len bytes.
template <class G>
SAM_HD void seqQual(const char *B, const char *Q, uint32_t len, uint32_t rc, uint64_t p, const G &g) {
    if (rc) {
        g.copy(p, (len + 1) / 2, [=](uint32_t k) {
            const uint32_t hi = seqCode(samline::complement(samline::upperCase(B[len - 1 - 2 * k])));
            const uint32_t lo = 2 * k + 1 < len ? seqCode(samline::complement(samline::upperCase(B[len - 2 - 2 * k]))) : 0u;
            return (char)(hi << 4 | lo);
        });
        g.copy(p + (len + 1) / 2, len, [=](uint32_t k) { return (char)(Q[len - 1 - k] - '!'); });
    } else {
        g.copy(p, (len + 1) / 2, [=](uint32_t k) {
            const uint32_t hi = seqCode(samline::upperCase(B[2 * k]));
            const uint32_t lo = 2 * k + 1 < len ? seqCode(samline::upperCase(B[2 * k + 1])) : 0u;
            return (char)(hi << 4 | lo);
        });
        g.copy(p + (len + 1) / 2, len, [=](uint32_t k) { return (char)(Q[k] - '!'); });
    }
}

// The tags at p: RG:Z (rg non-null), PG:Z:SNAP, NM:i = nm.  (rg ? 4 + rgLen : 0) + 15 bytes.
template <class G>
SAM_HD void tags(const char *rg, uint32_t rgLen, int32_t nm, uint64_t p, const G &g) {
    if (rg) {
        const char *tag = "RGZ";
        g.copy(p, 3, [=](uint32_t k) { return tag[k]; });
        g.copy(p + 3, rgLen, [=](uint32_t k) { return rg[k]; });
        if (g.lead()) g.put(p + 3 + rgLen, '\0');
        p += 4 + rgLen;
    }
    const char *tail = "PGZSNAP\0NMi";
    g.copy(p, 11, [=](uint32_t k) { return tail[k]; });
    if (g.lead()) put32(g, p + 11, (uint32_t)nm);
}

// The bytes of record i at output offset `at`: exactly recordLength(A, F) of them.  nm: the NM value
// (F.nmOwn, or the carried one where that is kNoNm).
template <class G>
SAM_HD void write(const Args &A, uint64_t i, const Fields &F, int32_t nm, uint64_t at, const G &g) {
    const uint32_t *ops = A.ops + i * SNAPGPU_CIGAR_MAX_OPS;
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
        put32(g, at + 24, 0xffffffffu);         // next_refID, next_pos: no mate
        put32(g, at + 28, 0xffffffffu);
        put32(g, at + 32, 0);                   // tlen
        g.put(at + 36 + F.qlen, '\0');
        // soft clips around the ops, mirrored for RC (as the SAM CIGAR, sam_line.h)
        uint64_t q = p;
        if (F.nCigar) {
            if (F.before) { put32(g, q, F.before << 4 | 4u); q += 4; }
            for (uint32_t k = 0; k < F.nOps; k++) { put32(g, q, ops[k]); q += 4; }
            if (F.after) put32(g, q, F.after << 4 | 4u);
        }
    }
    const char *id = A.ids + A.idOffsets[i];
    g.copy(at + 36, F.qlen, [=](uint32_t k) { return id[k]; });
    p += 4 * F.nCigar;
    seqQual(A.bases + F.readStart, A.quals + F.readStart, F.len, F.rc, p, g);
    p += (F.len + 1) / 2 + F.len;
    tags(A.rg, A.rgLen, nm, p, g);
}

using samline::Serial;

}  // namespace bamline
