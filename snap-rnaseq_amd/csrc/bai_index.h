// bai_index.h -- the rules of the BAI index (SAMv1 5.2) in the one canonical form the host model
// (host/bai.cpp) and the device passes (bai.hip) both write: a record's fields and reference span,
// virtual offsets, the chunk-head predicate, the sort keys and the byte sizes.  No rule is written
// anywhere else.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BAI_HD __host__ __device__ inline
#else
#define BAI_HD inline
#endif

namespace baiindex {

constexpr uint32_t kMemberIn = 0xff00;        // uncompressed bytes of every member the device compressor writes
constexpr uint32_t kPseudoBin = 37450;
constexpr uint32_t kWindowShift = 14;         // 16 kb linear-index windows
constexpr int64_t kMaxEnd = 1ll << 29;        // what the six-level binning scheme covers
constexpr uint32_t kMaxWindows = 1u << (29 - kWindowShift);
constexpr uint32_t kFixed = 36;               // block_size and the 32 fixed bytes
constexpr uint64_t kStreamOffsetLimit = 1ull << 48;
constexpr uint64_t kNoOffset = ~0ull;         // a window nobody overlaps, before the back-fill
constexpr uint32_t kHeaderBytes = 8, kTrailerBytes = 8;

BAI_HD uint32_t load16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
BAI_HD uint32_t load32(const uint8_t *p) { return load16(p) | load16(p + 2) << 16; }

// What the index reads of one record.  `bytes` = block_size + 4.
struct Fields {
    int32_t refID, pos;
    uint32_t bin, flag, nOps, nameLen;
};

BAI_HD Fields fields(const uint8_t *rec) {
    Fields f;
    f.refID = (int32_t)load32(rec + 4);
    f.pos = (int32_t)load32(rec + 8);
    f.nameLen = rec[12];
    f.bin = load16(rec + 14);
    f.nOps = load16(rec + 16);
    f.flag = load16(rec + 18);
    return f;
}

// A record of `bytes` bytes holds its fixed part and its CIGAR.
BAI_HD bool holdsCigar(const Fields &f, uint64_t bytes) { return bytes >= kFixed && kFixed + f.nameLen + 4ull * f.nOps <= bytes; }

// M, D, N, = and X advance the reference.
BAI_HD bool consumesReference(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// The reference bases a record covers: at least 1.  (holdsCigar held.)
BAI_HD int64_t span(const uint8_t *rec, const Fields &f) {
    const uint8_t *c = rec + kFixed + f.nameLen;
    int64_t s = 0;
    for (uint32_t k = 0; k < f.nOps; k++) {
        const uint32_t v = load32(c + 4 * k);
        if (consumesReference(v & 15)) s += v >> 4;
    }
    return s > 0 ? s : 1;
}

// Why a record is refused (0: it is not), apart from truncation and order.
enum Refusal : uint32_t { kOk = 0, kBadRef = 1, kBadPos = 2, kBadEnd = 3 };
BAI_HD uint32_t refusal(const Fields &f, int64_t end, int64_t nRef) {
    if (f.refID < -1 || f.refID >= nRef) return kBadRef;
    if (f.refID >= 0 && f.pos < 0) return kBadPos;
    if (f.refID >= 0 && end > kMaxEnd) return kBadEnd;
    return kOk;
}

// Records are in the ascending order of this key: (refID, pos), refID -1 last whatever its pos.
BAI_HD uint64_t sortKey(int32_t refID, int32_t pos) {
    return refID < 0 ? ~0ull : (uint64_t)(uint32_t)refID << 32 | (uint32_t)pos;
}

BAI_HD uint64_t voff(uint64_t streamOffset, uint64_t coff, uint32_t inMember) { return (streamOffset + coff) << 16 | inMember; }

// The device stream of `total` bytes: every member holds kMemberIn bytes, member m begins at coff[m],
// and coff of the member count is the stream's size -- so an offset that ends a member is offset 0 of
// the next, and the end of the data is where the EOF block goes.
BAI_HD uint64_t voffFixed(uint64_t streamOffset, const uint64_t *coff, uint64_t u, uint64_t total) {
    if (u >= total) return voff(streamOffset, coff[(total + kMemberIn - 1) / kMemberIn], 0);
    return voff(streamOffset, coff[u / kMemberIn], (uint32_t)(u % kMemberIn));
}

// A record with a reference begins a chunk when the record before it has another reference or bin.
BAI_HD bool chunkHead(bool first, int32_t prevRef, uint32_t prevBin, int32_t refID, uint32_t bin) {
    return refID >= 0 && (first || prevRef != refID || prevBin != bin);
}

// Chunks sort (stably) by this, 48 bits; a padding key sorts after every chunk.
constexpr uint32_t kChunkKeyBits = 48;
constexpr uint64_t kChunkKeyPad = (1ull << kChunkKeyBits) - 1;
BAI_HD uint64_t chunkKey(int32_t refID, uint32_t bin) { return (uint64_t)(uint32_t)refID << 16 | bin; }

BAI_HD uint32_t firstWindow(int32_t pos) { return (uint32_t)pos >> kWindowShift; }
BAI_HD uint32_t lastWindow(int64_t end) { return (uint32_t)((end - 1) >> kWindowShift); }

// Bytes of one reference's part: n_bin, the bins with their chunks, the pseudo-bin, n_intv, intervals.
BAI_HD uint64_t refBytes(bool hasRecords, uint64_t nBins, uint64_t nChunks, uint64_t nIntv) {
    return hasRecords ? 4 + nBins * 8 + nChunks * 16 + (8 + 32) + 4 + nIntv * 8 : 8;
}

// What an index of nRecords records (recordBytes bytes) over nRef references can take at most.
BAI_HD uint64_t sizeBound(uint64_t nRecords, uint64_t nRef, uint64_t recordBytes) {
    (void)recordBytes;
    const uint64_t withRecords = nRecords < nRef ? nRecords : nRef;
    return kHeaderBytes + nRef * 8 + withRecords * (40 + 8ull * kMaxWindows) + nRecords * 24 + kTrailerBytes;
}

}  // namespace baiindex
