// sam_format.h -- the device SAM formatter's kernels (sam_format.hip) as output_chain.hip launches them.
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

// A 64-lane wave as sam_line.h's group: bytes go to the LDS window [w0, w1) of the output.
struct Wave {
    char *lds;
    uint64_t w0, w1;
    uint32_t lane;
    template <class P>
    __device__ uint32_t firstOf(uint32_t n, P p) const {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t k = base + lane;
            const bool hit = k < n && p(k);
            const unsigned long long m = __ballot(hit);
            if (m) return base + (uint32_t)__ffsll(m) - 1;
        }
        return n;
    }
    template <class F>
    __device__ uint32_t sum(uint32_t n, F f) const {
        uint32_t s = 0;
        for (uint32_t k = lane; k < n; k += 64) s += f(k);
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        return s;
    }
    template <class F>
    __device__ void copy(uint64_t at, uint32_t n, F f) const {
        if (at + n <= w0 || at >= w1) return;
        for (uint32_t k = lane; k < n; k += 64) put(at + k, f(k));
    }
    __device__ void put(uint64_t at, char c) const {
        if (at >= w0 && at < w1) lds[at - w0] = c;
    }
    __device__ bool lead() const { return lane == 0; }
};

// The pieces of launch() that the paired SAM formatter (sam_pair_format.hip) and the BAM encoder
// (bam_format.hip) run as well, queued on st.
// sortStep: order fill, the stable radix sort of (S.key, record index) into S.order, and the gather
// S.slotLen[j] = len[S.order[j]]; S.keys is not read (the caller's length pass stored S.key).
// scanStarts: the exclusive 64-bit scan of n lengths into start[0 .. n], start[n] = their sum
// (sums: scanTiles(n) entries of scratch).
// checkLineEnds: *bad += the slots i < n that do not end in '\n' at start[i + 1] - 1, inside cap.
hipError_t sortStep(const SortBuffers &S, const uint32_t *len, uint64_t n, hipStream_t st);
void scanStarts(const uint32_t *len, uint64_t n, uint64_t *sums, uint64_t *start, hipStream_t st);
void checkLineEnds(const uint64_t *start, uint64_t n, const char *out, uint64_t cap, uint32_t *bad, hipStream_t st);

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
