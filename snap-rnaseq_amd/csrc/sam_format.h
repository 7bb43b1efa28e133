// sam_format.h -- the device SAM formatter's kernels (sam_format.hip) as aligner.hip launches them.
#pragma once
#include "sam_line.h"

#include <hip/hip_runtime.h>

namespace samgpu {

// The write pass: one workgroup per kRecsPerGroup consecutive records (one contiguous byte range of
// the text), staged in an LDS window of kTileBytes.  The scan: kScanTile lengths per workgroup.
// (snapgpu.SAM_RECORDS_PER_WORKGROUP / SAM_SCAN_TILE mirror the first and last for the tests.)
constexpr uint32_t kRecsPerGroup = 32;
constexpr uint32_t kTileBytes = 16384;
constexpr uint32_t kScanTile = 2048;

struct Buffers {
    uint32_t *len;     // [n]      line lengths
    samline::Scans *scans;   // [n]  what the length pass scanned, for the write pass
    uint64_t *start;   // [n + 1]  line starts; start[n] = bytes of text
    uint64_t *sums;    // [scanTiles(n)]
    char *text;        // textCap bytes, 16-byte aligned; a text that would not fit is not written
    uint64_t textCap;
    uint32_t *bad;     // lines whose last byte is not '\n' (always 0)
    hipEvent_t mid[2]; // recorded after the length pass and after the scan (per-pass timing), or null
};

// Coordinate-sorted output: what the sort step between the length pass and the scan needs.
struct SortBuffers {
    samline::SortArgs keys;      // the per-piece tables of samline::sortKey, on the device
    uint32_t *key, *keySorted;   // [n] each  samline::sortKey per record; the same, ascending
    uint32_t *iota, *order;      // [n] each  0 .. n - 1; order[j] = the record that output slot j prints
    uint32_t *slotLen;           // [n]       len[order[j]]: what the scan runs over
    void *temp;                  // sortTempBytes(n) of rocPRIM's temporary storage
    size_t tempBytes;
    hipEvent_t done;             // recorded after the sort step (its own timing), or null
};

inline uint64_t scanTiles(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }

// Bytes of temporary storage the radix sort of n (key, record) pairs on st asks for.  A size query
// on the host: nothing is launched and nothing is waited for.
hipError_t sortTempBytes(uint64_t n, hipStream_t st, size_t *bytes);

// Length pass, scan, write pass and the end-of-line check over n > 0 records, queued on st.
// S non-null: the lines in the stable order of their sort keys -- the length pass also stores the
// keys, a sort step (order fill, rocprim::radix_sort_pairs over 32 bits, gather of the lengths)
// follows it, the scan and the check run over output slots, and the write pass formats record
// S->order[j] into slot j.
hipError_t launch(const samline::Args &A, uint64_t n, const Buffers &B, hipStream_t st, const SortBuffers *S = nullptr);

}  // namespace samgpu
