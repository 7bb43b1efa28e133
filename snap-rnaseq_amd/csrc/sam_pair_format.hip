// sam_pair_format.hip -- SAM text of read pairs, written in HBM: sam_format.hip's passes over the
// 2n records of n pairs with sam_pair_line.h as the line rule.
//   length  one wave per record computes the exact byte length of its line;
//   scan    samgpu::scanStarts over the 2n lengths;
//   write   one workgroup per kRecsPerGroup consecutive records, their lines composed in an LDS
//           window of the text by one wave per record and flushed with 16-byte stores;
//   check   counts the lines that do not end in '\n' where the scan says they end.
// Record 2q + w is the w-th written end of pair q; which end that is, and its mate's fields, come
// from the pair record (samline::pairFields), so both waves of a pair read the same 64 bytes.
#include "sam_pair_format.h"

namespace sampairgpu {

using samgpu::kRecsPerGroup;
using samgpu::kTileBytes;
using samgpu::Wave;
using samline::PairArgs;
using samline::PairFields;

namespace {

__global__ __launch_bounds__(256) void pair_cigar_inputs_kernel(const snapgpu_pair_result_t *__restrict__ res, uint64_t nPairs,
                                                                uint32_t *__restrict__ outLocs, uint8_t *__restrict__ outDirs) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= nPairs) return;
    const snapgpu_pair_result_t p = res[q];
    for (uint32_t e = 0; e < 2; e++) {
        outLocs[e * nPairs + q] = p.status[e] != SNAPGPU_NOT_FOUND ? p.location[e] : samline::kInvalid;
        outDirs[e * nPairs + q] = p.direction[e];
    }
}

__global__ __launch_bounds__(256) void pair_length_kernel(PairArgs A, uint64_t n, uint32_t *__restrict__ len,
                                                          samline::Scans *__restrict__ scans) {
    const Wave g{nullptr, 0, 0, threadIdx.x & 63u};
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + threadIdx.x / 64u; r < n; r += waves) {
        const PairFields P = samline::pairFields(A, r, g);
        if (g.lane == 0) {
            len[r] = samline::pairLineLength(A, P);
            scans[r] = samline::Scans{P.F.qlen, (uint16_t)P.F.seqLen, (uint16_t)P.F.qualLen};   // both <= kMaxSeq
        }
    }
}

__global__ __launch_bounds__(256) void pair_write_kernel(PairArgs A, uint64_t n, const uint64_t *__restrict__ start,
                                                         const samline::Scans *__restrict__ scans,
                                                         char *__restrict__ out, uint64_t cap) {
    __shared__ uint4 tile[kTileBytes / 16];
    char *lds = reinterpret_cast<char *>(tile);
    const uint64_t first = (uint64_t)blockIdx.x * kRecsPerGroup;
    const uint64_t end = first + kRecsPerGroup < n ? first + kRecsPerGroup : n;
    const uint64_t r0 = start[first], r1 = start[end];
    if (r1 > cap) return;   // the host's bound on the text was too small: pair_check_kernel reports it
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    // windows are 16-byte aligned in the text, so an LDS chunk is a 16-byte aligned store
    for (uint64_t w0 = r0 & ~15ull; w0 < r1; w0 += kTileBytes) {
        const uint64_t w1 = w0 + kTileBytes < r1 ? w0 + kTileBytes : r1;
        const Wave g{lds, w0, w1, lane};
        for (uint64_t j = first + wave; j < end; j += 4) {
            const uint64_t s = start[j], e = start[j + 1];
            if (e <= w0 || s >= w1) continue;
            const samline::Scans known = scans[j];
            const PairFields P = samline::pairFields(A, j, g, &known);
            samline::pairWrite(A, j, P, s, g);
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

__global__ __launch_bounds__(256) void pair_check_kernel(const uint64_t *__restrict__ start, uint64_t n,
                                                         const char *__restrict__ out, uint64_t cap, uint32_t *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = start[i], e = start[i + 1];
    if (e <= s || e > cap || out[e - 1] != '\n') atomicAdd(bad, 1u);
}

}  // namespace

void cigarInputs(const snapgpu_pair_result_t *res, uint64_t nPairs, uint32_t *outLocs, uint8_t *outDirs, hipStream_t st) {
    hipLaunchKernelGGL(pair_cigar_inputs_kernel, dim3((unsigned)((nPairs + 255) / 256)), dim3(256), 0, st, res, nPairs, outLocs,
                       outDirs);
}

hipError_t launch(const PairArgs &A, uint64_t n, const samgpu::Buffers &B, hipStream_t st) {
    hipError_t e = hipMemsetAsync(B.bad, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint64_t nGroups = (n + kRecsPerGroup - 1) / kRecsPerGroup;
    const uint64_t lenBlocks = (n + 3) / 4 < 65536 ? (n + 3) / 4 : 65536;
    hipLaunchKernelGGL(pair_length_kernel, dim3((unsigned)lenBlocks), dim3(256), 0, st, A, n, B.len, B.scans);
    samgpu::scanStarts(B.len, n, B.sums, B.start, st);
    hipLaunchKernelGGL(pair_write_kernel, dim3((unsigned)nGroups), dim3(256), 0, st, A, n, B.start, B.scans, B.text,
                       B.textCap);
    hipLaunchKernelGGL(pair_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B.start, n, B.text,
                       B.textCap, B.bad);
    return hipGetLastError();
}

}  // namespace sampairgpu
