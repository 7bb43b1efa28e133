// bam_pair_format.hip -- BAM records of read pairs, encoded in HBM: the passes of bam_format.hip
// (bam_passes.h) over the 2n records of n pairs with bam_pair_line.h as the record rule.  The length
// and write kernels are line_passes.h's, instantiated for PairBamRule below; the NM carry passes and
// the block_size check are bam_format.hip's, the sort step and the scan sam_format.hip's.  Here:
// the pair rule's glue only.
// Record 2q + w is the w-th written end of pair q, so record order is the writer's order: the carry
// scan hands an end without location the NM of the record written before it, its mate's or an
// earlier pair's, and does so before the sort, as the reference's writer runs before its sort filter.
#include "bam_pair_format.h"

#include "bam_passes.h"

namespace bampairgpu {

using samgpu::Wave;
using samline::PairArgs;

namespace {

// The paired BAM record rule (bam_pair_line.h); the side is BamRule's.
struct PairBamRule {
    using Fields = bampairline::Fields;
    using Side = int32_t;
    struct SortTables {};
    PairArgs A;
    __device__ Fields fields(uint64_t r, const Wave &g) const { return bampairline::fields(A, r, g); }
    __device__ uint32_t length(const Fields &F) const { return bampairline::recordLength(A, F); }
    __device__ Side side(const Fields &F) const { return F.nmOwn; }
    __device__ uint32_t sortKey(const SortTables &, const Fields &F) const { return bampairline::sortKey(A, F); }
    __device__ void write(uint64_t r, uint64_t s, const Side *nm, const Wave &g) const {
        const Fields F = bampairline::fields(A, r, g);
        bampairline::write(A, r, F, nm[r], s, g);
    }
};

}  // namespace

hipError_t launch(const PairArgs &A, uint64_t n, int32_t nmCarryIn, const bamgpu::Buffers &B, hipStream_t st,
                  const samgpu::SortBuffers *S) {
    return bamgpu::launchRule<bampairline::kNoNm>(PairBamRule{A}, n, nmCarryIn, B, st, S);
}

}  // namespace bampairgpu
