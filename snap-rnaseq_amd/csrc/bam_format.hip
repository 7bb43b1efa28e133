// bam_format.hip -- BAM records of single-end alignments, encoded in HBM.
//
// The passes of sam_format.hip over n records whose reads, records and CIGAR ops are device resident,
// with bam_line.h as the line rule:
//   length  one wave per record computes its exact size and its own NM value, or "none" for a record
//           without CIGAR ops (and, for sorted output, its sort key);
//   carry   an inclusive "last defined value" scan of the NM values over input order, seeded with the
//           caller's carry-in: a record without ops repeats the NM of the record before it, as the
//           reference's writer does -- before its sort filter, so also input order for sorted output;
//   scan    samgpu::scanStarts over the sizes (over output slots after samgpu::sortStep when sorted);
//   write   one workgroup per kRecsPerGroup consecutive slots, one contiguous byte range: each wave
//           composes its records in an LDS window of that range (the lead lane writes the fixed part,
//           the CIGAR ops and the NM value, lanes copy id and QUAL bytes, lane k packs SEQ byte k)
//           and the workgroup flushes the window with 16-byte stores (staged_write.h).
// A last kernel counts the records whose block_size is not the size the scan gave them.
// The length and write kernels are line_passes.h's, instantiated for BamRule below; the NM carry
// passes and the block_size check are this file's own, and the paired encoder (bam_pair_format.hip)
// runs them too: bam_passes.h states the order of the passes once for both rules.
#include "bam_passes.h"
#include "bam_pair_line.h"

namespace bamgpu {

using samgpu::kScanTile;
using samgpu::Wave;
using samline::Args;

namespace {

// The BAM record rule (bam_line.h); its side is the record's own NM after the length pass, the NM
// it carries after the carry passes.  The sort key needs nothing beside the arguments.
struct BamRule {
    using Fields = bamline::Fields;
    using Side = int32_t;
    struct SortTables {};
    Args A;
    __device__ Fields fields(uint64_t r, const Wave &g) const { return bamline::fields(A, r, g); }
    __device__ uint32_t length(const Fields &F) const { return bamline::recordLength(A, F); }
    __device__ Side side(const Fields &F) const { return F.nmOwn; }
    __device__ uint32_t sortKey(const SortTables &, const Fields &F) const { return bamline::sortKey(A, F); }
    __device__ void write(uint64_t r, uint64_t s, const Side *nm, const Wave &g) const {
        const Fields F = bamline::fields(A, r, g);
        bamline::write(A, r, F, nm[r], s, g);
    }
};

constexpr uint32_t kPerThread = kScanTile / 256;

// The carry passes are templates over kNoNm, the rule's "no NM of its own" (bamline::kNoNm for reads
// without mate, bampairline::kNoNm for pairs, where -1 is an NM).

// the scan's operator: the later value where it is defined
template <int32_t kNoNm>
__device__ int32_t later(int32_t a, int32_t b) { return b != kNoNm ? b : a; }

// inclusive "last defined value" scan of sh[0 .. 256) in place
template <int32_t kNoNm>
__device__ void lastDefined256(int32_t *sh) {
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const int32_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : kNoNm;
        __syncthreads();
        sh[threadIdx.x] = later<kNoNm>(t, sh[threadIdx.x]);
        __syncthreads();
    }
}

// tiles[b] = the last defined NM of tile b, or kNoNm
template <int32_t kNoNm>
__global__ __launch_bounds__(256) void bam_nm_tile_last_kernel(const int32_t *__restrict__ nm, uint64_t n,
                                                               int32_t *__restrict__ tiles) {
    __shared__ int32_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kPerThread;
    int32_t v = kNoNm;
    for (uint32_t j = 0; j < kPerThread; j++)
        if (base + j < n) v = later<kNoNm>(v, nm[base + j]);
    sh[threadIdx.x] = v;
    __syncthreads();
    lastDefined256<kNoNm>(sh);
    if (threadIdx.x == 255) tiles[blockIdx.x] = sh[255];
}

// one workgroup: tiles[b] becomes the NM that enters tile b (carryIn before the first defined value)
template <int32_t kNoNm>
__global__ __launch_bounds__(256) void bam_nm_tiles_kernel(int32_t *__restrict__ tiles, uint64_t nTiles, int32_t carryIn) {
    __shared__ int32_t sh[256];
    int32_t carry = carryIn;
    for (uint64_t b0 = 0; b0 < nTiles; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        sh[threadIdx.x] = i < nTiles ? tiles[i] : kNoNm;
        __syncthreads();
        lastDefined256<kNoNm>(sh);
        const int32_t before = threadIdx.x ? sh[threadIdx.x - 1] : kNoNm, last = sh[255];
        if (i < nTiles) tiles[i] = before != kNoNm ? before : carry;
        if (last != kNoNm) carry = last;
        __syncthreads();
    }
}

// nm[i]: its own value, else the last defined one before it, else the value that enters its tile
template <int32_t kNoNm>
__global__ __launch_bounds__(256) void bam_nm_apply_kernel(int32_t *__restrict__ nm, uint64_t n,
                                                           const int32_t *__restrict__ tiles) {
    __shared__ int32_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kPerThread;
    int32_t v[kPerThread];
    int32_t t = kNoNm;
    for (uint32_t j = 0; j < kPerThread; j++) {
        v[j] = base + j < n ? nm[base + j] : kNoNm;
        t = later<kNoNm>(t, v[j]);
    }
    sh[threadIdx.x] = t;
    __syncthreads();
    lastDefined256<kNoNm>(sh);
    const int32_t before = threadIdx.x ? sh[threadIdx.x - 1] : kNoNm;
    int32_t cur = before != kNoNm ? before : tiles[blockIdx.x];
    for (uint32_t j = 0; j < kPerThread; j++) {
        if (v[j] != kNoNm) cur = v[j];
        if (base + j < n) nm[base + j] = cur;
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

template <int32_t kNoNm>
void nmCarry(int32_t *nm, uint64_t n, int32_t *nmTiles, int32_t carryIn, hipStream_t st) {
    const uint64_t nTiles = samgpu::scanTiles(n);
    const dim3 tiles((unsigned)nTiles);
    hipLaunchKernelGGL(bam_nm_tile_last_kernel<kNoNm>, tiles, dim3(256), 0, st, nm, n, nmTiles);
    hipLaunchKernelGGL(bam_nm_tiles_kernel<kNoNm>, dim3(1), dim3(256), 0, st, nmTiles, nTiles, carryIn);
    hipLaunchKernelGGL(bam_nm_apply_kernel<kNoNm>, tiles, dim3(256), 0, st, nm, n, nmTiles);
}
template void nmCarry<bamline::kNoNm>(int32_t *, uint64_t, int32_t *, int32_t, hipStream_t);
template void nmCarry<bampairline::kNoNm>(int32_t *, uint64_t, int32_t *, int32_t, hipStream_t);

void checkBlockSizes(const uint64_t *start, uint64_t n, const char *out, uint64_t cap, uint32_t *bad, hipStream_t st) {
    hipLaunchKernelGGL(bam_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, start, n, out, cap, bad);
}

hipError_t launch(const Args &A, uint64_t n, int32_t nmCarryIn, const Buffers &B, hipStream_t st,
                  const samgpu::SortBuffers *S) {
    return launchRule<bamline::kNoNm>(BamRule{A}, n, nmCarryIn, B, st, S);
}

}  // namespace bamgpu
