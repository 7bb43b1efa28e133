// dupmark_rule.h -- the rule of duplicate marking over a coordinate-sorted stream of single-end BAM
// records, in the one canonical form the host model (host/dupmark.cpp) and the device passes
// (dupmark.hip) both apply ("Duplicate marking on the device").  A record's fields, what
// the stream refuses and its order are bai_index.h's; no rule of the marking is written anywhere else.
#pragma once
#include "bai_index.h"

namespace duprule {

constexpr uint32_t kDupFlag = 0x400, kUnmappedFlag = 0x4, kReverseFlag = 0x10, kMateFlag = 0x1;
constexpr uint32_t kFlagHighByte = 19;          // the byte of a record that holds FLAG's bits 8-15
constexpr uint8_t kDupBit = kDupFlag >> 8;      // 0x400 within that byte
constexpr uint32_t kMaxSeq = 1u << 24;          // l_seq above it is refused: below, 254 * l_seq fits 32 bits
constexpr uint32_t kQualMissing = 0xff;         // a QUAL byte that counts 0

// Considered: the record has a location and is mapped.  (refID and pos passed baiindex::refusal.)
BAI_HD bool considered(const baiindex::Fields &f) { return f.refID >= 0 && f.pos >= 0 && !(f.flag & kUnmappedFlag); }
BAI_HD uint32_t strand(uint32_t flag) { return (flag & kReverseFlag) ? 1u : 0u; }

BAI_HD uint32_t seqLen(const uint8_t *rec) { return baiindex::load32(rec + 20); }

// Where QUAL begins in a record: behind the fixed part, the name, the CIGAR and the packed bases.
BAI_HD uint64_t qualOffset(const baiindex::Fields &f, uint32_t lSeq) {
    return baiindex::kFixed + f.nameLen + 4ull * f.nOps + ((uint64_t)lSeq + 1) / 2;
}
// A record of `bytes` bytes holds its bases and qualities.  (lSeq <= kMaxSeq.)
BAI_HD bool holdsQual(const baiindex::Fields &f, uint32_t lSeq, uint64_t bytes) { return qualOffset(f, lSeq) + lSeq <= bytes; }

BAI_HD uint32_t qualValue(uint32_t q) { return q == kQualMissing ? 0u : q; }
// The four QUAL bytes of one little-endian dword.
BAI_HD uint32_t qualValue4(uint32_t w) {
    return qualValue(w & 0xff) + qualValue((w >> 8) & 0xff) + qualValue((w >> 16) & 0xff) + qualValue(w >> 24);
}

// What a group keeps: the greatest of these -- the highest score, and among equal scores the earliest
// record of the stream (slot: the record's index, at most 0xfffffffe).  Never 0.
BAI_HD uint64_t rank(uint32_t score, uint32_t slot) { return (uint64_t)score << 32 | (0xffffffffu - slot); }

// The flag byte of a record that is marked or not: nothing but 0x400 changes.
BAI_HD uint8_t flagByte(uint8_t old, bool marked) { return marked ? (uint8_t)(old | kDupBit) : (uint8_t)(old & ~kDupBit); }

}  // namespace duprule
