// sam_line.h -- one SAM line of a read without mate and without transcriptome CIGAR, as
// samAppendLine (host/sam.cpp) prints it, restated over plain pointers for host and device:
// the exact length of record i's line, and a writer that stores exactly those bytes.
//
// Both parts are templates over a "group" G, the lanes that share one record:
//   g.firstOf(n, pred)  smallest k < n with pred(k), or n
//   g.sum(n, f)         f(0) + ... + f(n - 1)
//   g.copy(at, n, f)    byte f(k) to output offset at + k, every k < n
//   g.put(at, c)        one byte (called by the group's lead only)
//   g.lead()            the one lane that writes the short numeric fields
// Serial (below) is one host thread; sam_format.hip has the 64-lane wave that writes into an
// LDS window.  Every member of a group calls fields() / write() with the same arguments.
#pragma once
#include "snapgpu.h"

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAM_HD __host__ __device__ inline
#else
#define SAM_HD inline
#endif

namespace samline {

constexpr uint32_t kInvalid = 0xffffffffu;   // InvalidGenomeLocation
constexpr uint32_t kMaxSeq = 1024;           // the host formatter's SEQ / QUAL limit

// Inputs of n lines: the arguments of snapgpu_sam_format_clipped as plain arrays, the genome's
// pieces as offsets + a name blob (piece p's name = pieceNames[pieceNameOff[p] .. pieceNameOff[p + 1])).
struct Args {
    const char *bases, *quals;           // read i: [offsets[i], + lengths[i]) is the clipped read
    const uint64_t *offsets;
    const uint32_t *lengths;
    const uint32_t *front, *unclipped;   // Read::clip state per read, or both null (unclipped)
    const char *ids;
    const uint64_t *idOffsets;
    const uint32_t *idLengths;
    const snapgpu_result_t *res;
    const int32_t *ed;
    const uint32_t *nOps, *ops;          // rows of SNAPGPU_CIGAR_MAX_OPS
    const uint32_t *pieceOffsets;
    const uint32_t *pieceNameOff;
    const char *pieceNames;
    int32_t nPieces;
    uint32_t rgLen;
    const char *rg;                      // null: no RG:Z: tag
};

// What the coordinate-sort key (sortKey below) needs beside Args, per piece: the offset of the first
// piece that carries its name, and 1 where the name gives no location (empty, or it begins with '*').
// Kept out of Args: the unsorted kernels take Args by value and keep their arguments and their code.
struct SortArgs {
    const uint32_t *base;
    const uint8_t *none;
};

// What fields() decides about one line; write() places bytes by it.
struct Fields {
    uint64_t readStart;   // first byte of the unclipped read in bases / quals
    uint32_t qlen;        // QNAME: the id up to its first space
    uint32_t flags, pos, mapq;
    int32_t piece;        // -1: RNAME "*"
    uint32_t pieceLen;
    uint32_t cigar;       // 1: soft clips + ops; 0: "*"
    uint32_t cigarLen, before, after, nOps;
    int32_t ed;           // the NM value
    uint32_t fullLen, seqLen, qualLen, rc;
};

SAM_HD char upperCase(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 0x20) : c; }   // Tables.cpp:74-80
SAM_HD char complement(char c) {                                                          // Tables.cpp:22-30
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': return 'A';
        case 'N': return 'N';
        case 'n': return 'n';
        default: return 0;
    }
}

SAM_HD uint32_t decLen(uint64_t v) {
    uint32_t k = 1;
    while (v >= 10) { v /= 10; k++; }
    return k;
}
SAM_HD uint32_t intLen(int64_t v) { return v < 0 ? 1 + decLen((uint64_t)(-v)) : decLen((uint64_t)v); }

// Genome::getPieceAtLocation (Genome.cpp:357-374)
SAM_HD int32_t pieceAt(const uint32_t *po, int32_t np, uint32_t loc) {
    int32_t lo = 0, hi = np - 1;
    while (lo <= hi) {
        const int32_t mid = (lo + hi) / 2;
        if (po[mid] <= loc && (mid == np - 1 || po[mid + 1] > loc)) return mid;
        else if (po[mid] <= loc) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// The three scans of a line (QNAME's first space, the NUL that ends SEQ, the one that ends QUAL):
// the device length pass keeps them for the write pass.
struct Scans {
    uint32_t qlen;
    uint16_t seqLen, qualLen;
};

// RNAME and POS of record i alone (F.piece, F.pieceLen, F.pos) -> the location getSAMData prints
// them from: NotFound -> unmapped (kInvalid).  Reads A.res and the pieces only, for a caller that
// has no reads or ids (snapgpu_sam_sort_keys).  fields() below sets the same three members by the
// same statements, inline as they always were: the device kernels' code depends on their order.
SAM_HD uint32_t locate(const Args &A, uint64_t i, Fields &F) {
    uint32_t loc = A.res[i].location;
    if (A.res[i].result == SNAPGPU_NOT_FOUND) loc = kInvalid;
    F.piece = -1;
    F.pieceLen = 1;
    F.pos = 0;
    if (loc != kInvalid) {
        const int32_t p = pieceAt(A.pieceOffsets, A.nPieces, loc);
        if (p >= 0) {
            F.piece = p;
            F.pieceLen = A.pieceNameOff[p + 1] - A.pieceNameOff[p];
            F.pos = loc - A.pieceOffsets[p] + 1;
        }
    }
    return loc;
}

// The coordinate-sort key of the line F prints: SAMFormat::getSortInfo's location (SAM.cpp:639-685),
// as the host sorter (samSortKey, host/sam.cpp) reads it back from RNAME and POS -- kInvalid for
// RNAME "*" and for a piece name that is empty or begins with '*', else the offset of the first
// piece of that name + POS - 1 (uint32_t arithmetic).  F needs locate() only.
SAM_HD uint32_t sortKey(const SortArgs &K, const Fields &F) {
    if (F.piece < 0 || K.none[F.piece]) return kInvalid;
    return K.base[F.piece] + F.pos - 1u;
}

template <class G>
SAM_HD Fields fields(const Args &A, uint64_t i, const G &g, const Scans *known = nullptr) {
    Fields F;
    const uint32_t front = A.front ? A.front[i] : 0u;
    const uint32_t clipped = A.lengths[i];
    F.fullLen = A.unclipped ? A.unclipped[i] : clipped;
    F.readStart = A.offsets[i] - front;
    // getSAMData: NotFound -> unmapped, unmapped -> forward
    const uint32_t recLoc = A.res[i].location;
    uint32_t loc = recLoc;
    if (A.res[i].result == SNAPGPU_NOT_FOUND) loc = kInvalid;
    F.rc = loc != kInvalid && A.res[i].direction == SNAPGPU_RC;
    F.flags = 0;
    F.mapq = 0;
    F.piece = -1;
    F.pieceLen = 1;
    F.pos = 0;
    if (loc != kInvalid) {
        if (F.rc) F.flags |= 0x10;   // SAM_REVERSE_COMPLEMENT
        const int32_t p = pieceAt(A.pieceOffsets, A.nPieces, loc);
        if (p >= 0) {
            F.piece = p;
            F.pieceLen = A.pieceNameOff[p + 1] - A.pieceNameOff[p];
            F.pos = loc - A.pieceOffsets[p] + 1;
        }
        int32_t m = A.res[i].mapq;
        m = m > 70 ? 70 : m;
        F.mapq = (uint32_t)(m < 0 ? 0 : m);
    } else {
        F.flags |= 0x04;             // SAM_UNMAPPED
    }
    const char *id = A.ids + A.idOffsets[i];
    F.qlen = known ? known->qlen : g.firstOf(A.idLengths[i], [=](uint32_t k) { return id[k] == ' '; });
    // CIGAR and NM at writeRead's own location, even for NotFound (SAM.cpp:1041-1066)
    F.ed = recLoc != kInvalid ? A.ed[i] : -1;
    F.cigar = recLoc != kInvalid && F.ed >= 0;
    const uint32_t back = F.fullLen - clipped - front;
    F.before = F.rc ? back : front;
    F.after = F.rc ? front : back;
    F.nOps = A.nOps[i] < SNAPGPU_CIGAR_MAX_OPS ? A.nOps[i] : SNAPGPU_CIGAR_MAX_OPS;   // a row holds no more
    F.cigarLen = 1;
    if (F.cigar) {
        const uint32_t *ops = A.ops + i * SNAPGPU_CIGAR_MAX_OPS;
        F.cigarLen = (F.before ? decLen(F.before) + 1 : 0) + (F.after ? decLen(F.after) + 1 : 0) +
                     g.sum(F.nOps, [=](uint32_t k) { return decLen(ops[k] >> 4) + 1; });
    }
    // SEQ / QUAL are printed with "%.*s" (SAM.cpp:1122-1136): a NUL byte ends them early
    const uint32_t len = F.fullLen, n = len < kMaxSeq ? len : kMaxSeq;
    const char *B = A.bases + F.readStart, *Q = A.quals + F.readStart;
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
    return F;
}

// bytes from QNAME to the tab before SEQ, after RNAME: "\t" POS "\t" MAPQ "\t" CIGAR "\t*\t0\t0\t"
SAM_HD uint32_t midLen(const Fields &F) { return 1 + decLen(F.pos) + 1 + decLen(F.mapq) + 1 + F.cigarLen + 7; }

SAM_HD uint32_t lineLength(const Args &A, const Fields &F) {
    return F.qlen + 1 + decLen(F.flags) + 1 + F.pieceLen + midLen(F) + F.seqLen + 1 + F.qualLen +
           (A.rg ? 6 + A.rgLen : 0) + 16 + intLen(F.ed) + 1;
}

template <class G>
SAM_HD uint64_t putU(const G &g, uint64_t at, uint64_t v) {
    const uint32_t k = decLen(v);
    for (uint32_t j = k; j-- > 0;) { g.put(at + j, (char)('0' + v % 10)); v /= 10; }
    return at + k;
}

// The bytes of line i at output offset `at`: exactly lineLength(A, F) of them.
template <class G>
SAM_HD void write(const Args &A, uint64_t i, const Fields &F, uint64_t at, const G &g) {
    const char *id = A.ids + A.idOffsets[i];
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
    if (g.lead()) {
        uint64_t q = p;
        g.put(q++, '\t');
        q = putU(g, q, F.pos);
        g.put(q++, '\t');
        q = putU(g, q, F.mapq);
        g.put(q++, '\t');
        if (F.cigar) {
            // soft clips around the CIGAR (computeCigarString, SAM.cpp:1212-1226), mirrored for RC
            const uint32_t *ops = A.ops + i * SNAPGPU_CIGAR_MAX_OPS;
            if (F.before) { q = putU(g, q, F.before); g.put(q++, 'S'); }
            for (uint32_t k = 0; k < F.nOps; k++) {
                q = putU(g, q, ops[k] >> 4);
                g.put(q++, "MIDNSHP=X"[ops[k] & 15]);
            }
            if (F.after) { q = putU(g, q, F.after); g.put(q++, 'S'); }
        } else {
            g.put(q++, '*');
        }
    }
    p += midLen(F) - 7;
    const char *mate = "\t*\t0\t0\t";
    g.copy(p, 7, [=](uint32_t k) { return mate[k]; });
    p += 7;
    const uint32_t len = F.fullLen;
    const char *B = A.bases + F.readStart, *Q = A.quals + F.readStart;
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
        uint64_t q = p;
        int64_t v = F.ed;
        if (v < 0) { g.put(q++, '-'); v = -v; }
        g.put(putU(g, q, (uint64_t)v), '\n');
    }
}

// One host thread as the whole group, writing at out[offset].
struct Serial {
    char *out;
    template <class P>
    uint32_t firstOf(uint32_t n, P p) const {
        for (uint32_t k = 0; k < n; k++)
            if (p(k)) return k;
        return n;
    }
    template <class F>
    uint32_t sum(uint32_t n, F f) const {
        uint32_t s = 0;
        for (uint32_t k = 0; k < n; k++) s += f(k);
        return s;
    }
    template <class F>
    void copy(uint64_t at, uint32_t n, F f) const {
        for (uint32_t k = 0; k < n; k++) out[at + k] = f(k);
    }
    void put(uint64_t at, char c) const { out[at] = c; }
    bool lead() const { return true; }
};

}  // namespace samline
