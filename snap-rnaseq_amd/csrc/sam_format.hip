// sam_format.hip -- SAM text of single-end records, written in HBM.
//
// Three passes over n records whose reads, records and CIGAR ops are device resident:
//   length  one wave per record computes the exact byte length of its line (sam_line.h);
//   scan    exclusive scan of the lengths into 64-bit line starts, start[n] = bytes of text;
//   write   one workgroup per kRecsPerGroup consecutive records.  Their lines are one contiguous
//           byte range of the text: each wave composes its records' lines in an LDS window of that
//           range (lanes copy id, SEQ and QUAL bytes in parallel, lane 0 prints the few numbers),
//           then the workgroup flushes the window with 16-byte lane-contiguous stores (the range's
//           unaligned head and tail bytewise).  Nothing is stored outside [start[first], start[end)).
// A last kernel counts the lines that do not end in '\n' where the scan says they end.
//
// Coordinate-sorted output (-so) is the same passes over output slots: the length pass also stores
// each record's sort key, a stable radix sort of (key, record index) gives order[slot] = record, the
// scan runs over the lengths gathered in that order, and the write pass formats record order[j]
// into slot j.  A workgroup still owns kRecsPerGroup consecutive slots, one contiguous byte range.
#include "sam_format.h"

#include <cstring>
#include <rocprim/rocprim.hpp>

namespace samgpu {

using samline::Args;
using samline::Fields;

namespace {

// What only the sorted instances of the length and write kernels take, as their last argument: the
// unsorted instances get an empty one, and keep the arguments they had before there was a sorted
// launch (and with them their registers and code).
template <bool Sorted>
struct KeyOut {};
template <>
struct KeyOut<true> {
    samline::SortArgs tables;
    uint32_t *key;   // [n] out: samline::sortKey per record
};
template <bool Sorted>
struct SlotOrder {
    __device__ uint64_t record(uint64_t j) const { return j; }
};
template <>
struct SlotOrder<true> {
    const uint32_t *order;   // [n] output slot -> record
    __device__ uint64_t record(uint64_t j) const { return order[j]; }
};

// Sorted: key[r] = the record's coordinate-sort key as well
template <bool Sorted>
__global__ __launch_bounds__(256) void sam_length_kernel(Args A, uint64_t n, uint32_t *__restrict__ len,
                                                         samline::Scans *__restrict__ scans, KeyOut<Sorted> K) {
    const Wave g{nullptr, 0, 0, threadIdx.x & 63u};
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + threadIdx.x / 64u; r < n; r += waves) {
        const Fields F = samline::fields(A, r, g);
        if (g.lane == 0) {
            len[r] = samline::lineLength(A, F);
            scans[r] = samline::Scans{F.qlen, (uint16_t)F.seqLen, (uint16_t)F.qualLen};   // both <= kMaxSeq
            if constexpr (Sorted) K.key[r] = samline::sortKey(K.tables, F);
        }
    }
}

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

// Sorted: start[] is over output slots and slot j prints record O.order[j] (scans[] stays per
// record), else slot j prints record j.
template <bool Sorted>
__global__ __launch_bounds__(256) void sam_write_kernel(Args A, uint64_t n, const uint64_t *__restrict__ start,
                                                        const samline::Scans *__restrict__ scans,
                                                        char *__restrict__ out, uint64_t cap, SlotOrder<Sorted> O) {
    __shared__ uint4 tile[kTileBytes / 16];
    char *lds = reinterpret_cast<char *>(tile);
    const uint64_t first = (uint64_t)blockIdx.x * kRecsPerGroup;
    const uint64_t end = first + kRecsPerGroup < n ? first + kRecsPerGroup : n;
    const uint64_t r0 = start[first], r1 = start[end];
    if (r1 > cap) return;   // the host's bound on the text was too small: sam_check_kernel reports it
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    // windows are 16-byte aligned in the text, so an LDS chunk is a 16-byte aligned store
    for (uint64_t w0 = r0 & ~15ull; w0 < r1; w0 += kTileBytes) {
        const uint64_t w1 = w0 + kTileBytes < r1 ? w0 + kTileBytes : r1;
        const Wave g{lds, w0, w1, lane};
        for (uint64_t j = first + wave; j < end; j += 4) {
            const uint64_t s = start[j], e = start[j + 1];
            if (e <= w0 || s >= w1) continue;
            const uint64_t r = O.record(j);
            if (Sorted && r >= n) continue;   // not a record (never): the slot is empty, the check reports it
            const samline::Scans known = scans[r];
            const Fields F = samline::fields(A, r, g, &known);
            samline::write(A, r, F, s, g);
        }
        __syncthreads();
        const uint32_t chunks = (uint32_t)((w1 - w0 + 15) / 16);
        for (uint32_t c = threadIdx.x; c < chunks; c += 256) {
            const uint64_t a = w0 + 16ull * c;
            if (a >= r0 && a + 16 <= r1) {
                *reinterpret_cast<uint4 *>(out + a) = tile[c];
            } else {
                const uint64_t lo = a > r0 ? a : r0, hi = a + 16 < r1 ? a + 16 : r1;
                for (uint64_t b = lo; b < hi; b++) out[b] = lds[b - w0];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void sam_check_kernel(const uint64_t *__restrict__ start, uint64_t n,
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
    const dim3 perItem((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(sam_iota_kernel, perItem, dim3(256), 0, st, S.iota, n);
    size_t bytes = S.tempBytes;
    hipError_t e = sortPairs(S.temp, bytes, &S, n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sam_gather_len_kernel, perItem, dim3(256), 0, st, len, S.order, n, S.slotLen);
    return S.done ? hipEventRecord(S.done, st) : hipSuccess;
}

void scanStarts(const uint32_t *len, uint64_t n, uint64_t *sums, uint64_t *start, hipStream_t st) {
    const uint64_t nTiles = scanTiles(n);
    hipLaunchKernelGGL(sam_scan_sums_kernel, dim3((unsigned)nTiles), dim3(256), 0, st, len, n, sums);
    hipLaunchKernelGGL(sam_scan_tiles_kernel, dim3(1), dim3(256), 0, st, sums, nTiles, start + n);
    hipLaunchKernelGGL(sam_scan_starts_kernel, dim3((unsigned)nTiles), dim3(256), 0, st, len, n, sums, start);
}

hipError_t launch(const Args &A, uint64_t n, const Buffers &B, hipStream_t st, const SortBuffers *S) {
    hipError_t e = hipMemsetAsync(B.bad, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint64_t nGroups = (n + kRecsPerGroup - 1) / kRecsPerGroup;
    const uint64_t lenBlocks = (n + 3) / 4 < 65536 ? (n + 3) / 4 : 65536;
    const dim3 perItem((unsigned)((n + 255) / 256));
    if (S) hipLaunchKernelGGL(sam_length_kernel<true>, dim3((unsigned)lenBlocks), dim3(256), 0, st, A, n, B.len, B.scans,
                              KeyOut<true>{S->keys, S->key});
    else hipLaunchKernelGGL(sam_length_kernel<false>, dim3((unsigned)lenBlocks), dim3(256), 0, st, A, n, B.len, B.scans,
                            KeyOut<false>{});
    if (B.mid[0] && (e = hipEventRecord(B.mid[0], st)) != hipSuccess) return e;
    const uint32_t *len = B.len;
    if (S) {
        if ((e = sortStep(*S, B.len, n, st)) != hipSuccess) return e;
        len = S->slotLen;
    }
    scanStarts(len, n, B.sums, B.start, st);
    if (B.mid[1] && (e = hipEventRecord(B.mid[1], st)) != hipSuccess) return e;
    if (S) hipLaunchKernelGGL(sam_write_kernel<true>, dim3((unsigned)nGroups), dim3(256), 0, st, A, n, B.start, B.scans,
                              B.text, B.textCap, SlotOrder<true>{S->order});
    else hipLaunchKernelGGL(sam_write_kernel<false>, dim3((unsigned)nGroups), dim3(256), 0, st, A, n, B.start, B.scans,
                            B.text, B.textCap, SlotOrder<false>{});
    hipLaunchKernelGGL(sam_check_kernel, perItem, dim3(256), 0, st, B.start, n, B.text, B.textCap, B.bad);
    return hipGetLastError();
}

}  // namespace samgpu
