// fastq_parse.h -- the device FASTQ parser's kernels (fastq_parse.hip) as fastq_upload.hip launches them.
#pragma once
#include "fastq_record.h"

#include <hip/hip_runtime.h>

namespace fqgpu {

// The newline passes: one workgroup of 256 lanes per kTileBytes of text, 64 bytes (four 16-byte
// loads) per lane.  The copy pass: one workgroup per kRecsPerGroup consecutive records, each of its
// three outputs staged in an LDS window of kStageBytes.
constexpr uint32_t kTileBytes = 16384;
constexpr uint32_t kRecsPerGroup = 32;
constexpr uint32_t kStageBytes = 16384;

inline uint64_t tiles(uint64_t nBytes) { return (nBytes + kTileBytes - 1) / kTileBytes; }
// The text buffer's size: the kernels load whole 64-byte lane spans, and expect zero bytes from
// nBytes to the end of the buffer.
inline uint64_t textCapacity(uint64_t nBytes) { return ((nBytes + 63) & ~63ull) + 64; }

struct Totals {
    unsigned long long firstBad;    // the first record without '@' header (starts as all ones)
    unsigned long long baseBytes;   // sum of the records' base lengths (starts as 0)
    uint32_t maxBaseLen, maxIdLen;  // the longest unclipped read and the longest id (start as 0; limits())
};

struct Records {   // [n] each
    uint32_t *idLen, *baseLen, *qualLen;
    uint32_t *front, *clipLen;   // Read::clip of the record: front clip and clipped length
};

// counts[t] = '\n' bytes in tile t (tiles(nBytes) > 0 tiles)
void countNewlines(const char *text, uint64_t nBytes, uint32_t *counts, hipStream_t st);
// nl[k] = position of the k-th '\n'; tileStart[t] = '\n' bytes before tile t (the scan of counts)
void lineStarts(const char *text, uint64_t nBytes, const uint64_t *tileStart, uint64_t *nl, uint64_t nNl, hipStream_t st);
// fastq_record.h over records 0 .. n (n > 0), a wave per record; *tot as initialised above
void records(const char *text, uint64_t nBytes, const uint64_t *nl, uint64_t nNl, uint64_t n, int clipping,
             const Records &R, Totals *tot, hipStream_t st);
// tot->maxBaseLen / maxIdLen = the largest of baseLen[0 .. n) / idLen[0 .. n) (n > 0): what the device
// form of the SAM / BAM calls checks in place of the host loops over a host batch
void limits(const uint32_t *baseLen, const uint32_t *idLen, uint64_t n, Totals *tot, hipStream_t st);
// ids, bases and qualities (0x00 where the quality line is shorter) to ids[idStart[r] ..],
// bases / quals[baseStart[r] ..]; offsets[r] / lengths[r] = the clipped extent
void pack(const char *text, uint64_t nBytes, const uint64_t *nl, uint64_t nNl, uint64_t n, const Records &R,
          const uint64_t *baseStart, const uint64_t *idStart, char *bases, char *quals, char *ids,
          uint64_t *offsets, uint32_t *lengths, hipStream_t st);

}  // namespace fqgpu
