// sam_pair_format.h -- the device formatter of paired SAM records (sam_pair_format.hip) as
// paired_output.hip launches it.  It shares sam_format.h's buffers, wave group, scan and sizes.
#pragma once
#include "sam_format.h"
#include "sam_pair_line.h"

namespace sampairgpu {

// cigar_kernel's explicit locations and directions for the ends of n pairs, from the pair records:
// entry e * n + q = location[e] of pair q (invalid where NotFound) and direction[e], so each end's
// n entries go with that end's resident reads in a launch of its own.
void cigarInputs(const snapgpu_pair_result_t *res, uint64_t nPairs, uint32_t *outLocs, uint8_t *outDirs, hipStream_t st);

// Length pass, samgpu::scanStarts, write pass and the end-of-line check over nRecords = 2n > 0
// records, queued on st (B.mid is not recorded).
hipError_t launch(const samline::PairArgs &A, uint64_t nRecords, const samgpu::Buffers &B, hipStream_t st);

}  // namespace sampairgpu
