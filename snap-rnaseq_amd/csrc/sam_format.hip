// sam_format.hip -- SAM text of single-end records, written in HBM.
//
// Three passes over n records whose reads, records and CIGAR ops are device resident:
//   length  one wave per record computes the exact byte length of its line (sam_line.h);
//   scan    exclusive scan of the lengths into 64-bit line starts, start[n] = bytes of text;
//   write   one workgroup per kRecsPerGroup consecutive records, their lines one contiguous byte range
//           of the text: each wave composes its records' lines in an LDS window of that range (lanes
//           copy id, SEQ and QUAL bytes in parallel, lane 0 prints the few numbers) and the workgroup
//           flushes the window with 16-byte stores (staged_write.h).
// A last kernel counts the lines that do not end in '\n' where the scan says they end.
// The length and write kernels are line_passes.h's, instantiated for SamRule below; the scan, the
// sort step and the end-of-line check are defined here and serve the paired SAM formatter
// (sam_pair_format.hip) and the BAM encoder (bam_format.hip) as well.
//
// Coordinate-sorted output (-so) is the same passes over output slots: the length pass also stores
// each record's sort key, a stable radix sort of (key, record index) gives order[slot] = record, the
// scan runs over the lengths gathered in that order, and the write pass formats record order[j]
// into slot j.  A workgroup still owns kRecsPerGroup consecutive slots, one contiguous byte range.
#include "line_passes.h"

#include <cstring>
#include <rocprim/rocprim.hpp>

namespace samgpu {

using samline::Args;

namespace {

// The single-end SAM line rule (sam_line.h); its side is what the length pass scanned of the
// record, which the write pass does not scan again.
struct SamRule {
    using Fields = samline::Fields;
    using Side = samline::Scans;
    using SortTables = samline::SortArgs;
    Args A;
    __device__ Fields fields(uint64_t r, const Wave &g) const { return samline::fields(A, r, g); }
    __device__ uint32_t length(const Fields &F) const { return samline::lineLength(A, F); }
    __device__ Side side(const Fields &F) const { return Side{F.qlen, (uint16_t)F.seqLen, (uint16_t)F.qualLen}; }   // both <= kMaxSeq
    __device__ uint32_t sortKey(const SortTables &tables, const Fields &F) const { return samline::sortKey(tables, F); }
    __device__ void write(uint64_t r, uint64_t s, const Side *scans, const Wave &g) const {
        const samline::Scans known = scans[r];
        const Fields F = samline::fields(A, r, g, &known);
        samline::write(A, r, F, s, g);
    }
};

// the sort's values before it runs: record j in slot j
__global__ __launch_bounds__(256) void sam_iota_kernel(uint32_t *__restrict__ iota, uint64_t n) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j < n) iota[j] = (uint32_t)j;
}

// slotLen[j] = len[order[j]]: the scan's input in output order (order holds a permutation of 0 .. n - 1;
// an index that is not below n -- never -- reads nothing and gives a length the check kernel reports)
__global__ __launch_bounds__(256) void sam_gather_len_kernel(const uint32_t *__restrict__ len,
                                                             const uint32_t *__restrict__ order, uint64_t n,
                                                             uint32_t *__restrict__ slotLen) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = order[j];
    slotLen[j] = r < n ? len[r] : 0u;
}

constexpr uint32_t kPerThread = kScanTile / 256;

// sums[b] = sum of tile b's lengths
__global__ __launch_bounds__(256) void sam_scan_sums_kernel(const uint32_t *__restrict__ len, uint64_t n,
                                                            uint64_t *__restrict__ sums) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kPerThread;
    uint64_t s = 0;
    for (uint32_t j = 0; j < kPerThread; j++)
        if (base + j < n) s += len[base + j];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t o = 128; o; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

// inclusive scan of sh[0 .. 256) in place
__device__ void scan256(uint64_t *sh) {
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint64_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
}

// one workgroup: the tile sums become the tiles' first starts; *total = bytes of text
__global__ __launch_bounds__(256) void sam_scan_tiles_kernel(uint64_t *__restrict__ sums, uint64_t nTiles,
                                                             uint64_t *__restrict__ total) {
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < nTiles; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t v = i < nTiles ? sums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        scan256(sh);
        if (i < nTiles) sums[i] = carry + sh[threadIdx.x] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void sam_scan_starts_kernel(const uint32_t *__restrict__ len, uint64_t n,
                                                              const uint64_t *__restrict__ sums,
                                                              uint64_t *__restrict__ start) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kPerThread;
    uint32_t v[kPerThread];
    uint64_t s = 0;
    for (uint32_t j = 0; j < kPerThread; j++) {
        v[j] = base + j < n ? len[base + j] : 0u;
        s += v[j];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    scan256(sh);
    uint64_t at = sums[blockIdx.x] + sh[threadIdx.x] - s;
    for (uint32_t j = 0; j < kPerThread; j++) {
        if (base + j < n) start[base + j] = at;
        at += v[j];
    }
}

// Slot i of the output ends in '\n' where the scan says it ends
__global__ __launch_bounds__(256) void line_ends_check_kernel(const uint64_t *__restrict__ start, uint64_t n,
                                                              const char *__restrict__ out, uint64_t cap,
                                                              uint32_t *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = start[i], e = start[i + 1];
    if (e <= s || e > cap || out[e - 1] != '\n') atomicAdd(bad, 1u);
}

}  // namespace

// rocPRIM's radix sort is stable in each of its algorithms (one workgroup, a merge of block-sorted
// runs, onesweep passes): equal keys keep their input order, as std::stable_sort does in the host sorter.
static hipError_t sortPairs(void *temp, size_t &bytes, const SortBuffers *S, uint64_t n, hipStream_t st) {
    return rocprim::radix_sort_pairs(temp, bytes, S ? S->key : (uint32_t *)nullptr, S ? S->keySorted : (uint32_t *)nullptr,
                                     S ? S->iota : (uint32_t *)nullptr, S ? S->order : (uint32_t *)nullptr, (size_t)n,
                                     0u, 32u, st);
}

hipError_t sortTempBytes(uint64_t n, hipStream_t st, size_t *bytes) {
    *bytes = 0;
    return sortPairs(nullptr, *bytes, nullptr, n, st);
}

hipError_t sortStep(const SortBuffers &S, const uint32_t *len, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(sam_iota_kernel, perItem(n), dim3(256), 0, st, S.iota, n);
    size_t bytes = S.tempBytes;
    hipError_t e = sortPairs(S.temp, bytes, &S, n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sam_gather_len_kernel, perItem(n), dim3(256), 0, st, len, S.order, n, S.slotLen);
    return S.done ? hipEventRecord(S.done, st) : hipSuccess;
}

void scanStarts(const uint32_t *len, uint64_t n, uint64_t *sums, uint64_t *start, hipStream_t st) {
    const uint64_t nTiles = scanTiles(n);
    hipLaunchKernelGGL(sam_scan_sums_kernel, dim3((unsigned)nTiles), dim3(256), 0, st, len, n, sums);
    hipLaunchKernelGGL(sam_scan_tiles_kernel, dim3(1), dim3(256), 0, st, sums, nTiles, start + n);
    hipLaunchKernelGGL(sam_scan_starts_kernel, dim3((unsigned)nTiles), dim3(256), 0, st, len, n, sums, start);
}

void checkLineEnds(const uint64_t *start, uint64_t n, const char *out, uint64_t cap, uint32_t *bad, hipStream_t st) {
    hipLaunchKernelGGL(line_ends_check_kernel, perItem(n), dim3(256), 0, st, start, n, out, cap, bad);
}

hipError_t launch(const Args &A, uint64_t n, const Buffers &B, hipStream_t st, const SortBuffers *S) {
    const SamRule R{A};
    hipError_t e = S ? lengthPass(R, n, B.len, B.scans, B.bad, st, KeyOut<true, SamRule>{S->keys, S->key})
                     : lengthPass(R, n, B.len, B.scans, B.bad, st, KeyOut<false, SamRule>{});
    if (e != hipSuccess) return e;
    if (B.mid[0] && (e = hipEventRecord(B.mid[0], st)) != hipSuccess) return e;
    const uint32_t *len = B.len;
    if (S) {
        if ((e = sortStep(*S, B.len, n, st)) != hipSuccess) return e;
        len = S->slotLen;
    }
    scanStarts(len, n, B.sums, B.start, st);
    if (B.mid[1] && (e = hipEventRecord(B.mid[1], st)) != hipSuccess) return e;
    if (S) writePass(R, n, B.start, B.scans, B.text, B.textCap, st, SlotOrder<true>{S->order});
    else writePass(R, n, B.start, B.scans, B.text, B.textCap, st, SlotOrder<false>{});
    checkLineEnds(B.start, n, B.text, B.textCap, B.bad, st);
    return hipGetLastError();
}

}  // namespace samgpu
