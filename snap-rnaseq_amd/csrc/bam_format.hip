// bam_format.hip -- BAM records of single-end alignments, encoded in HBM.
//
// The passes of sam_format.hip over n records whose reads, records and CIGAR ops are device resident,
// with bam_line.h in place of sam_line.h:
//   length  one wave per record computes its exact size and its own NM value, or "none" for a record
//           without CIGAR ops (and, for sorted output, its sort key);
//   carry   an inclusive "last defined value" scan of the NM values over input order, seeded with the
//           caller's carry-in: a record without ops repeats the NM of the record before it, as the
//           reference's writer does -- before its sort filter, so also input order for sorted output;
//   scan    samgpu::scanStarts over the sizes (over output slots after samgpu::sortStep when sorted);
//   write   one workgroup per kRecsPerGroup consecutive slots, one contiguous byte range: each wave
//           composes its records in an LDS window of that range (the lead lane writes the fixed part,
//           the CIGAR ops and the NM value, lanes copy id and QUAL bytes, lane k packs SEQ byte k),
//           then the workgroup flushes the window with 16-byte lane-contiguous stores (the range's
//           unaligned head and tail bytewise).  Nothing is stored outside [start[first], start[end)).
// A last kernel counts the records whose block_size is not the size the scan gave them.
#include "bam_format.h"

namespace bamgpu {

using bamline::Fields;
using bamline::kNoNm;
using samgpu::kRecsPerGroup;
using samgpu::kScanTile;
using samgpu::kTileBytes;
using samgpu::Wave;
using samline::Args;

namespace {

template <bool Sorted>
struct KeyOut {};
template <>
struct KeyOut<true> {
    uint32_t *key;   // [n] out: bamline::sortKey per record
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

template <bool Sorted>
__global__ __launch_bounds__(256) void bam_length_kernel(Args A, uint64_t n, uint32_t *__restrict__ len,
                                                         int32_t *__restrict__ nm, KeyOut<Sorted> K) {
    const Wave g{nullptr, 0, 0, threadIdx.x & 63u};
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + threadIdx.x / 64u; r < n; r += waves) {
        const Fields F = bamline::fields(A, r, g);
        if (g.lane == 0) {
            len[r] = bamline::recordLength(A, F);
            nm[r] = F.nmOwn;
            if constexpr (Sorted) K.key[r] = bamline::sortKey(A, F);
        }
    }
}

constexpr uint32_t kPerThread = kScanTile / 256;

// the scan's operator: the later value where it is defined
__device__ int32_t later(int32_t a, int32_t b) { return b != kNoNm ? b : a; }

// inclusive "last defined value" scan of sh[0 .. 256) in place
__device__ void lastDefined256(int32_t *sh) {
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const int32_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : kNoNm;
        __syncthreads();
        sh[threadIdx.x] = later(t, sh[threadIdx.x]);
        __syncthreads();
    }
}

// tiles[b] = the last defined NM of tile b, or kNoNm
__global__ __launch_bounds__(256) void bam_nm_tile_last_kernel(const int32_t *__restrict__ nm, uint64_t n,
                                                               int32_t *__restrict__ tiles) {
    __shared__ int32_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kPerThread;
    int32_t v = kNoNm;
    for (uint32_t j = 0; j < kPerThread; j++)
        if (base + j < n) v = later(v, nm[base + j]);
    sh[threadIdx.x] = v;
    __syncthreads();
    lastDefined256(sh);
    if (threadIdx.x == 255) tiles[blockIdx.x] = sh[255];
}

// one workgroup: tiles[b] becomes the NM that enters tile b (carryIn before the first defined value)
__global__ __launch_bounds__(256) void bam_nm_tiles_kernel(int32_t *__restrict__ tiles, uint64_t nTiles, int32_t carryIn) {
    __shared__ int32_t sh[256];
    int32_t carry = carryIn;
    for (uint64_t b0 = 0; b0 < nTiles; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        sh[threadIdx.x] = i < nTiles ? tiles[i] : kNoNm;
        __syncthreads();
        lastDefined256(sh);
        const int32_t before = threadIdx.x ? sh[threadIdx.x - 1] : kNoNm, last = sh[255];
        if (i < nTiles) tiles[i] = before != kNoNm ? before : carry;
        if (last != kNoNm) carry = last;
        __syncthreads();
    }
}

// nm[i]: its own value, else the last defined one before it, else the value that enters its tile
__global__ __launch_bounds__(256) void bam_nm_apply_kernel(int32_t *__restrict__ nm, uint64_t n,
                                                           const int32_t *__restrict__ tiles) {
    __shared__ int32_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kPerThread;
    int32_t v[kPerThread];
    int32_t t = kNoNm;
    for (uint32_t j = 0; j < kPerThread; j++) {
        v[j] = base + j < n ? nm[base + j] : kNoNm;
        t = later(t, v[j]);
    }
    sh[threadIdx.x] = t;
    __syncthreads();
    lastDefined256(sh);
    const int32_t before = threadIdx.x ? sh[threadIdx.x - 1] : kNoNm;
    int32_t cur = before != kNoNm ? before : tiles[blockIdx.x];
    for (uint32_t j = 0; j < kPerThread; j++) {
        if (v[j] != kNoNm) cur = v[j];
        if (base + j < n) nm[base + j] = cur;
    }
}

// Sorted: start[] is over output slots and slot j holds record O.order[j] (nm[] stays per record),
// else slot j holds record j.
template <bool Sorted>
__global__ __launch_bounds__(256) void bam_write_kernel(Args A, uint64_t n, const uint64_t *__restrict__ start,
                                                        const int32_t *__restrict__ nm, char *__restrict__ out,
                                                        uint64_t cap, SlotOrder<Sorted> O) {
    __shared__ uint4 tile[kTileBytes / 16];
    char *lds = reinterpret_cast<char *>(tile);
    const uint64_t first = (uint64_t)blockIdx.x * kRecsPerGroup;
    const uint64_t end = first + kRecsPerGroup < n ? first + kRecsPerGroup : n;
    const uint64_t r0 = start[first], r1 = start[end];
    if (r1 > cap) return;   // the host's bound on the output was too small: bam_check_kernel reports it
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    // windows are 16-byte aligned in the output, so an LDS chunk is a 16-byte aligned store
    for (uint64_t w0 = r0 & ~15ull; w0 < r1; w0 += kTileBytes) {
        const uint64_t w1 = w0 + kTileBytes < r1 ? w0 + kTileBytes : r1;
        const Wave g{lds, w0, w1, lane};
        for (uint64_t j = first + wave; j < end; j += 4) {
            const uint64_t s = start[j], e = start[j + 1];
            if (e <= w0 || s >= w1) continue;
            const uint64_t r = O.record(j);
            if (Sorted && r >= n) continue;   // not a record (never): the slot is empty, the check reports it
            const Fields F = bamline::fields(A, r, g);
            bamline::write(A, r, F, nm[r], s, g);
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

// block_size of slot i must be its scanned size - 4, at its scanned start
__global__ __launch_bounds__(256) void bam_check_kernel(const uint64_t *__restrict__ start, uint64_t n,
                                                        const char *__restrict__ out, uint64_t cap, uint32_t *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = start[i], e = start[i + 1];
    bool ok = e >= s + 36 && e <= cap;
    if (ok) {
        uint32_t blockSize = 0;
        for (uint32_t k = 0; k < 4; k++) blockSize |= (uint32_t)(uint8_t)out[s + k] << (8 * k);
        ok = blockSize == e - s - 4;
    }
    if (!ok) atomicAdd(bad, 1u);
}

}  // namespace

hipError_t launch(const Args &A, uint64_t n, int32_t nmCarryIn, const Buffers &B, hipStream_t st,
                  const samgpu::SortBuffers *S) {
    hipError_t e = hipMemsetAsync(B.bad, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint64_t nTiles = samgpu::scanTiles(n), nGroups = (n + kRecsPerGroup - 1) / kRecsPerGroup;
    const uint64_t lenBlocks = (n + 3) / 4 < 65536 ? (n + 3) / 4 : 65536;
    const dim3 perItem((unsigned)((n + 255) / 256)), tiles((unsigned)nTiles);
    if (S) hipLaunchKernelGGL(bam_length_kernel<true>, dim3((unsigned)lenBlocks), dim3(256), 0, st, A, n, B.len, B.nm,
                              KeyOut<true>{S->key});
    else hipLaunchKernelGGL(bam_length_kernel<false>, dim3((unsigned)lenBlocks), dim3(256), 0, st, A, n, B.len, B.nm,
                            KeyOut<false>{});
    hipLaunchKernelGGL(bam_nm_tile_last_kernel, tiles, dim3(256), 0, st, B.nm, n, B.nmTiles);
    hipLaunchKernelGGL(bam_nm_tiles_kernel, dim3(1), dim3(256), 0, st, B.nmTiles, nTiles, nmCarryIn);
    hipLaunchKernelGGL(bam_nm_apply_kernel, tiles, dim3(256), 0, st, B.nm, n, B.nmTiles);
    const uint32_t *len = B.len;
    if (S) {
        if ((e = samgpu::sortStep(*S, B.len, n, st)) != hipSuccess) return e;
        len = S->slotLen;
    }
    samgpu::scanStarts(len, n, B.sums, B.start, st);
    if (S) hipLaunchKernelGGL(bam_write_kernel<true>, dim3((unsigned)nGroups), dim3(256), 0, st, A, n, B.start, B.nm, B.out,
                              B.outCap, SlotOrder<true>{S->order});
    else hipLaunchKernelGGL(bam_write_kernel<false>, dim3((unsigned)nGroups), dim3(256), 0, st, A, n, B.start, B.nm, B.out,
                            B.outCap, SlotOrder<false>{});
    hipLaunchKernelGGL(bam_check_kernel, perItem, dim3(256), 0, st, B.start, n, B.out, B.outCap, B.bad);
    return hipGetLastError();
}

}  // namespace bamgpu
