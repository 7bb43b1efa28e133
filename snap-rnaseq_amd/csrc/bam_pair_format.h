// bam_pair_format.h -- the device BAM encoder for read pairs (bam_pair_format.hip) as
// paired_output.hip launches it.
#pragma once
#include "bam_format.h"
#include "bam_pair_line.h"

namespace bampairgpu {

// bamgpu::launch over the n > 0 records of n / 2 pairs (record 2q + w is the w-th written end of pair
// q) with bam_pair_line.h as the rule, queued on st: length pass, NM carry from nmCarryIn over write
// order, scan, write pass and the block_size check.  S non-null: the records in the stable order of
// bampairline::sortKey (S->keys is not used); the carry still runs over write order.
hipError_t launch(const samline::PairArgs &A, uint64_t n, int32_t nmCarryIn, const bamgpu::Buffers &B, hipStream_t st,
                  const samgpu::SortBuffers *S = nullptr);

}  // namespace bampairgpu
