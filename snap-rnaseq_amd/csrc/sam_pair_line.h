// sam_pair_line.h -- the two SAM lines of a read pair without transcriptome CIGAR, as the paired
// writer prints them (host/rna_paired.cpp's record loop over samAppendLine with SamLine::hasMate,
// host/sam.cpp), restated over plain pointers for host and device like sam_line.h, whose group
// interface, helpers, Fields and Scans it uses: the exact length of record j's line, and a writer
// that stores exactly those bytes.
//
// Pair q of n gives records 2q and 2q + 1 (SimpleReadWriter::writePair, ReadWriter.cpp:133-217):
// with locs[e] = location[e], or invalid where status[e] is NotFound, the end written first is
// first = locs[0] > locs[1] (equal locations keep end 0 first); record 2q + w is the w-th written
// end.  The CIGAR arrays have 2n rows, one for end e of pair q whichever is written first: row
// q * rowPair + e * rowEnd (2q + e in the public layout; q + e * n where each end's rows are a plane).
// The mate fields are getSAMData's hasMate branch (SAM.cpp:914-973).
#pragma once
#include "sam_line.h"

namespace samline {

// Inputs of the 2n lines of n pairs: per end the arrays of Args, one record array, the CIGAR rows.
struct PairArgs {
    const char *bases[2], *quals[2];       // end e of pair q: [offsets[e][q], + lengths[e][q]) is the clipped read
    const uint64_t *offsets[2];
    const uint32_t *lengths[2];
    const uint32_t *front[2], *unclipped[2];   // Read::clip state per end, or both null (that end unclipped)
    const char *ids[2];
    const uint64_t *idOffsets[2];
    const uint32_t *idLengths[2];
    const snapgpu_pair_result_t *res;      // [n]
    const int32_t *ed;                     // [2n]
    const uint32_t *nOps, *ops;            // [2n] rows of SNAPGPU_CIGAR_MAX_OPS
    uint64_t rowPair, rowEnd;              // end e of pair q is row q * rowPair + e * rowEnd
    const uint32_t *pieceOffsets;
    const uint32_t *pieceNameOff;
    const char *pieceNames;
    int32_t nPieces;
    uint32_t rgLen;
    const char *rg;                        // null: no RG:Z: tag
};

// What pairFields() decides about one line: F as for a read without mate (flags, RNAME and POS
// already with the mate's part), and the three mate fields.
struct PairFields {
    Fields F;
    uint32_t end;         // the end this record prints
    uint32_t idLen;       // that end's id after the "/1" "/2" trim (QNAME is its first F.qlen bytes)
    int32_t matePiece;    // RNEXT: a piece's name, -1 "*", -2 "="
    uint32_t mateLen;
    uint32_t pnext;
    int64_t tlen;
};

// the end record j prints and its pair's locations (invalid where NotFound)
SAM_HD uint32_t pairEnd(const PairArgs &A, uint64_t j, uint32_t locs[2]) {
    const snapgpu_pair_result_t &r = A.res[j >> 1];
    for (int k = 0; k < 2; k++) locs[k] = r.status[k] != SNAPGPU_NOT_FOUND ? r.location[k] : kInvalid;
    const uint32_t first = locs[0] > locs[1];
    return (j & 1) == 0 ? first : 1u - first;
}

// What pairPlace() hands on beside the fields: the record's own and its mate's location (invalid
// where NotFound), and whether both lie on one piece.
struct PairPlace {
    uint32_t loc, mateLoc;
    bool onePiece;
};

// Where record j and its mate lie, from the pair record and the piece offsets alone: P.end, and of
// F the strand, FLAG, MAPQ, the piece and POS (already with the mate's part), RNEXT and PNEXT
// (getSAMData's hasMate branch, SAM.cpp:914-973).  The BAM pair rule (bam_pair_line.h) starts here too.
SAM_HD PairPlace pairPlace(const PairArgs &A, uint64_t j, PairFields &P) {
    Fields &F = P.F;
    const snapgpu_pair_result_t &r = A.res[j >> 1];
    uint32_t locs[2];
    const uint32_t e = pairEnd(A, j, locs), m = 1u - e;
    P.end = e;
    // getSAMData: NotFound -> unmapped, unmapped -> forward
    const uint32_t loc = locs[e], mateLoc = locs[m];
    F.rc = loc != kInvalid && r.direction[e] == SNAPGPU_RC;
    F.flags = 0;
    F.mapq = 0;
    F.piece = -1;
    F.pos = 0;
    int32_t pieceIdx = -1;
    if (loc != kInvalid) {
        if (F.rc) F.flags |= 0x10;   // SAM_REVERSE_COMPLEMENT
        const int32_t p = pieceAt(A.pieceOffsets, A.nPieces, loc);
        if (p >= 0) {
            F.piece = pieceIdx = p;
            F.pos = loc - A.pieceOffsets[p] + 1;
        }
        int32_t mq = r.mapq[e];
        mq = mq > 70 ? 70 : mq;
        F.mapq = (uint32_t)(mq < 0 ? 0 : mq);
    } else {
        F.flags |= 0x04;             // SAM_UNMAPPED
    }
    // mate fields (SAM.cpp:914-973): RNEXT "=" unless both are mapped on different pieces
    F.flags |= 0x01 | ((j & 1) == 0 ? 0x40 : 0x80);   // SAM_MULTI_SEGMENT, SAM_FIRST_SEGMENT / SAM_LAST_SEGMENT
    P.matePiece = -1;
    P.pnext = 0;
    int32_t mateIdx = -1;
    if (mateLoc != kInvalid) {
        const int32_t mp = pieceAt(A.pieceOffsets, A.nPieces, mateLoc);
        if (mp >= 0) {
            P.matePiece = mateIdx = mp;
            P.pnext = mateLoc - A.pieceOffsets[mp] + 1;
        }
        if (r.direction[m] == SNAPGPU_RC) F.flags |= 0x20;   // SAM_NEXT_REVERSED
        if (loc == kInvalid) {       // the unmapped end takes the mate's RNAME / POS
            F.piece = mp >= 0 ? mp : -1;
            pieceIdx = -2;           // never the mate's piece below
            P.matePiece = -2;
            F.pos = P.pnext;
        }
    } else {
        F.flags |= 0x08;             // SAM_NEXT_UNMAPPED
        P.matePiece = -2;
        P.pnext = F.pos;
    }
    if (loc != kInvalid && mateLoc != kInvalid) F.flags |= 0x02;   // SAM_ALL_ALIGNED
    const bool onePiece = pieceIdx >= 0 && pieceIdx == mateIdx;
    if (onePiece) P.matePiece = -2;
    return PairPlace{loc, mateLoc, onePiece};
}

// The piece index behind RNEXT: where P.matePiece says "=", the piece the record itself names.
SAM_HD int32_t pairMateIndex(const PairFields &P) { return P.matePiece == -2 ? P.F.piece : P.matePiece; }

// The unclipped read of the end pairPlace() chose, its soft clips as the strand mirrors them, and
// TLEN from the clipped-read extents of both ends.
SAM_HD void pairExtents(const PairArgs &A, uint64_t j, const PairPlace &L, PairFields &P) {
    Fields &F = P.F;
    const uint64_t q = j >> 1;
    const snapgpu_pair_result_t &r = A.res[q];
    const uint32_t e = P.end, m = 1u - e;
    const uint32_t front = A.front[e] ? A.front[e][q] : 0u;
    const uint32_t clipped = A.lengths[e][q];
    F.fullLen = A.unclipped[e] ? A.unclipped[e][q] : clipped;
    F.readStart = A.offsets[e][q] - front;
    const uint32_t back = F.fullLen - clipped - front;
    F.before = F.rc ? back : front;
    F.after = F.rc ? front : back;
    P.tlen = 0;
    if (L.loc != kInvalid && L.mateLoc != kInvalid) {
        const uint32_t loc = L.loc, mateLoc = L.mateLoc;
        const uint32_t mFront = A.front[m] ? A.front[m][q] : 0u, mClipped = A.lengths[m][q];
        const uint32_t mFull = A.unclipped[m] ? A.unclipped[m][q] : mClipped;
        const int64_t myStart = (int64_t)(uint32_t)(loc - F.before);
        const int64_t myEnd = (int64_t)(uint32_t)(loc + clipped + F.after);
        const int64_t mBefore = mFront, mAfter = (int64_t)mFull - mClipped - mFront;
        const int64_t mateStart = (int64_t)mateLoc - (r.direction[m] == SNAPGPU_RC ? mAfter : mBefore);
        const int64_t mateEnd = (int64_t)mateLoc + mClipped + (r.direction[m] == SNAPGPU_FORWARD ? mAfter : mBefore);
        if (L.onePiece) P.tlen = myStart < mateStart ? mateEnd - myStart : -(myEnd - mateStart);
    }
}

// Length of end e's id of pair q once writePair has dropped "/1" and "/2" from both ids (the
// condition as rna_paired.cpp has it).
SAM_HD uint32_t pairIdLen(const PairArgs &A, uint64_t q, uint32_t e) {
    uint32_t idLen[2] = {A.idLengths[0][q], A.idLengths[1][q]};
    const char *id0 = A.ids[0] + A.idOffsets[0][q], *id1 = A.ids[1] + A.idOffsets[1][q];
    if (idLen[0] == idLen[1] && idLen[0] > 2 && id0[idLen[0] - 2] == '/' && id1[idLen[0] - 2] == '/') {
        const char c0 = id0[idLen[0] - 1], c1 = id1[idLen[1] - 1];
        if ((c0 == '1' || c0 == '2') && (c0 == '1' || c1 == '2') && c0 != c1) { idLen[0] -= 2; idLen[1] -= 2; }
    }
    return idLen[e];
}

template <class G>
SAM_HD PairFields pairFields(const PairArgs &A, uint64_t j, const G &g, const Scans *known = nullptr) {
    PairFields P;
    Fields &F = P.F;
    const uint64_t q = j >> 1;
    const PairPlace L = pairPlace(A, j, P);
    pairExtents(A, j, L, P);
    const uint32_t e = P.end, loc = L.loc;
    F.pieceLen = F.piece >= 0 ? A.pieceNameOff[F.piece + 1] - A.pieceNameOff[F.piece] : 1u;
    P.mateLen = P.matePiece >= 0 ? A.pieceNameOff[P.matePiece + 1] - A.pieceNameOff[P.matePiece] : 1u;
    // QNAME: the trimmed id ends at its first space
    P.idLen = pairIdLen(A, q, e);
    const char *id = A.ids[e] + A.idOffsets[e][q];
    const uint32_t idN = P.idLen;
    F.qlen = known ? known->qlen : g.firstOf(idN, [=](uint32_t k) { return id[k] == ' '; });
    // CIGAR and NM only at a location (the paired writer passes the invalid one for NotFound)
    const uint64_t row = q * A.rowPair + e * A.rowEnd;
    F.ed = loc != kInvalid ? A.ed[row] : -1;
    F.cigar = loc != kInvalid && F.ed >= 0;
    F.nOps = A.nOps[row] < SNAPGPU_CIGAR_MAX_OPS ? A.nOps[row] : SNAPGPU_CIGAR_MAX_OPS;   // a row holds no more
    F.cigarLen = 1;
    if (F.cigar) {
        const uint32_t *ops = A.ops + row * SNAPGPU_CIGAR_MAX_OPS;
        F.cigarLen = (F.before ? decLen(F.before) + 1 : 0) + (F.after ? decLen(F.after) + 1 : 0) +
                     g.sum(F.nOps, [=](uint32_t k) { return decLen(ops[k] >> 4) + 1; });
    }
    // SEQ / QUAL are printed with "%.*s" (SAM.cpp:1122-1136): a NUL byte ends them early
    const uint32_t len = F.fullLen, n = len < kMaxSeq ? len : kMaxSeq;
    const char *B = A.bases[e] + F.readStart, *Q = A.quals[e] + F.readStart;
    if (known) {
        F.seqLen = known->seqLen;
        F.qualLen = known->qualLen;
    } else if (F.rc) {
        F.seqLen = g.firstOf(n, [=](uint32_t k) { return complement(upperCase(B[len - 1 - k])) == 0; });
        F.qualLen = g.firstOf(n, [=](uint32_t k) { return Q[len - 1 - k] == 0; });
    } else {
        F.seqLen = g.firstOf(n, [=](uint32_t k) { return B[k] == 0; });
        F.qualLen = g.firstOf(n, [=](uint32_t k) { return Q[k] == 0; });
    }
    return P;
}

// bytes after RNAME up to the tab before SEQ: "\t" POS "\t" MAPQ "\t" CIGAR "\t" RNEXT "\t" PNEXT "\t" TLEN "\t"
SAM_HD uint32_t pairMidLen(const PairFields &P) {
    return 1 + decLen(P.F.pos) + 1 + decLen(P.F.mapq) + 1 + P.F.cigarLen + 1 + P.mateLen + 1 + decLen(P.pnext) + 1 +
           intLen(P.tlen) + 1;
}

SAM_HD uint32_t pairLineLength(const PairArgs &A, const PairFields &P) {
    const Fields &F = P.F;
    return F.qlen + 1 + decLen(F.flags) + 1 + F.pieceLen + pairMidLen(P) + F.seqLen + 1 + F.qualLen +
           (A.rg ? 6 + A.rgLen : 0) + 16 + intLen(F.ed) + 1;
}

// The bytes of record j's line at output offset `at`: exactly pairLineLength(A, P) of them.
template <class G>
SAM_HD void pairWrite(const PairArgs &A, uint64_t j, const PairFields &P, uint64_t at, const G &g) {
    const Fields &F = P.F;
    const uint64_t q = j >> 1;
    const uint32_t e = P.end;
    const char *id = A.ids[e] + A.idOffsets[e][q];
    g.copy(at, F.qlen, [=](uint32_t k) { return id[k]; });
    uint64_t p = at + F.qlen;
    if (g.lead()) {
        g.put(p, '\t');
        g.put(putU(g, p + 1, F.flags), '\t');
    }
    p += 1 + decLen(F.flags) + 1;
    const char *name = F.piece >= 0 ? A.pieceNames + A.pieceNameOff[F.piece] : "*";
    g.copy(p, F.pieceLen, [=](uint32_t k) { return name[k]; });
    p += F.pieceLen;
    const uint32_t toMate = 1 + decLen(F.pos) + 1 + decLen(F.mapq) + 1 + F.cigarLen + 1;
    if (g.lead()) {
        uint64_t w = p;
        g.put(w++, '\t');
        w = putU(g, w, F.pos);
        g.put(w++, '\t');
        w = putU(g, w, F.mapq);
        g.put(w++, '\t');
        if (F.cigar) {
            // soft clips around the CIGAR (computeCigarString, SAM.cpp:1212-1226), mirrored for RC
            const uint32_t *ops = A.ops + (q * A.rowPair + e * A.rowEnd) * SNAPGPU_CIGAR_MAX_OPS;
            if (F.before) { w = putU(g, w, F.before); g.put(w++, 'S'); }
            for (uint32_t k = 0; k < F.nOps; k++) {
                w = putU(g, w, ops[k] >> 4);
                g.put(w++, "MIDNSHP=X"[ops[k] & 15]);
            }
            if (F.after) { w = putU(g, w, F.after); g.put(w++, 'S'); }
        } else {
            g.put(w++, '*');
        }
        g.put(w, '\t');
    }
    p += toMate;
    const char *mate = P.matePiece >= 0 ? A.pieceNames + A.pieceNameOff[P.matePiece] : P.matePiece == -2 ? "=" : "*";
    g.copy(p, P.mateLen, [=](uint32_t k) { return mate[k]; });
    p += P.mateLen;
    if (g.lead()) {
        uint64_t w = p;
        g.put(w++, '\t');
        w = putU(g, w, P.pnext);
        g.put(w++, '\t');
        int64_t v = P.tlen;
        if (v < 0) { g.put(w++, '-'); v = -v; }
        g.put(putU(g, w, (uint64_t)v), '\t');
    }
    p += 1 + decLen(P.pnext) + 1 + intLen(P.tlen) + 1;
    const uint32_t len = F.fullLen;
    const char *B = A.bases[e] + F.readStart, *Q = A.quals[e] + F.readStart;
    if (F.rc) {
        g.copy(p, F.seqLen, [=](uint32_t k) { return complement(upperCase(B[len - 1 - k])); });
        g.copy(p + F.seqLen + 1, F.qualLen, [=](uint32_t k) { return Q[len - 1 - k]; });
    } else {
        g.copy(p, F.seqLen, [=](uint32_t k) { return upperCase(B[k]); });
        g.copy(p + F.seqLen + 1, F.qualLen, [=](uint32_t k) { return Q[k]; });
    }
    if (g.lead()) g.put(p + F.seqLen, '\t');
    p += F.seqLen + 1 + F.qualLen;
    if (A.rg) {
        const char *tag = "\tRG:Z:", *rg = A.rg;
        g.copy(p, 6, [=](uint32_t k) { return tag[k]; });
        g.copy(p + 6, A.rgLen, [=](uint32_t k) { return rg[k]; });
        p += 6 + A.rgLen;
    }
    const char *tail = "\tPG:Z:SNAP\tNM:i:";
    g.copy(p, 16, [=](uint32_t k) { return tail[k]; });
    p += 16;
    if (g.lead()) {
        uint64_t w = p;
        int64_t v = F.ed;
        if (v < 0) { g.put(w++, '-'); v = -v; }
        g.put(putU(g, w, (uint64_t)v), '\n');
    }
}

}  // namespace samline
