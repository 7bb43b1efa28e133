// sam_pair_format.hip -- SAM text of read pairs, written in HBM: the passes of sam_format.hip over
// the 2n records of n pairs with sam_pair_line.h as the line rule.  The length and write kernels are
// line_passes.h's, instantiated for PairRule below; the scan and the end-of-line check are
// sam_format.hip's.  Here: the pair rule's glue, and the kernel that turns the pair records into
// cigar_kernel's inputs.
// Record 2q + w is the w-th written end of pair q; which end that is, and its mate's fields, come
// from the pair record (samline::pairFields), so both waves of a pair read the same 64 bytes.
#include "sam_pair_format.h"

#include "line_passes.h"

namespace sampairgpu {

using samgpu::Wave;
using samline::PairArgs;

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

// The paired SAM line rule (sam_pair_line.h); the side is SamRule's.
struct PairRule {
    using Fields = samline::PairFields;
    using Side = samline::Scans;
    PairArgs A;
    __device__ Fields fields(uint64_t r, const Wave &g) const { return samline::pairFields(A, r, g); }
    __device__ uint32_t length(const Fields &P) const { return samline::pairLineLength(A, P); }
    __device__ Side side(const Fields &P) const { return Side{P.F.qlen, (uint16_t)P.F.seqLen, (uint16_t)P.F.qualLen}; }   // both <= kMaxSeq
    __device__ void write(uint64_t r, uint64_t s, const Side *scans, const Wave &g) const {
        const samline::Scans known = scans[r];
        const Fields P = samline::pairFields(A, r, g, &known);
        samline::pairWrite(A, r, P, s, g);
    }
};

}  // namespace

void cigarInputs(const snapgpu_pair_result_t *res, uint64_t nPairs, uint32_t *outLocs, uint8_t *outDirs, hipStream_t st) {
    hipLaunchKernelGGL(pair_cigar_inputs_kernel, dim3((unsigned)((nPairs + 255) / 256)), dim3(256), 0, st, res, nPairs, outLocs,
                       outDirs);
}

hipError_t launch(const PairArgs &A, uint64_t n, const samgpu::Buffers &B, hipStream_t st) {
    const PairRule R{A};
    const hipError_t e = samgpu::lengthPass(R, n, B.len, B.scans, B.bad, st, samgpu::KeyOut<false, PairRule>{});
    if (e != hipSuccess) return e;
    samgpu::scanStarts(B.len, n, B.sums, B.start, st);
    samgpu::writePass(R, n, B.start, B.scans, B.text, B.textCap, st, samgpu::SlotOrder<false>{});
    samgpu::checkLineEnds(B.start, n, B.text, B.textCap, B.bad, st);
    return hipGetLastError();
}

}  // namespace sampairgpu
