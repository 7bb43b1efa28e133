// bam_format.h -- the device BAM encoder's kernels (bam_format.hip) as output_chain.hip launches them.
#pragma once
#include "bam_line.h"
#include "sam_format.h"

namespace bamgpu {

// The work split is the SAM formatter's: samgpu::kRecsPerGroup slots per workgroup of the write
// pass, an LDS window of samgpu::kTileBytes, samgpu::kScanTile values per workgroup of both scans.
struct Buffers {
    uint32_t *len;      // [n]      record sizes (block_size + 4)
    int32_t *nm;        // [n]      in: each record's own NM or bamline::kNoNm; out: the NM it carries
    int32_t *nmTiles;   // [scanTiles(n)]
    uint64_t *start;    // [n + 1]  record starts over output slots; start[n] = bytes of output
    uint64_t *sums;     // [scanTiles(n)]
    char *out;          // outCap bytes, 16-byte aligned; an output that would not fit is not written
    uint64_t outCap;
    uint32_t *bad;      // records whose block_size is not what the scan gave them (always 0)
};

// Length pass, NM carry, scan, write pass and the block_size check over n > 0 records, queued on st.
// The NM carry runs over input order and starts from nmCarryIn.  S non-null: the records in the
// stable order of bamline::sortKey -- the length pass stores the keys in S->key, samgpu::sortStep
// orders them, the size scan and the check run over output slots, and the write pass encodes record
// S->order[j] into slot j (S->keys is not used).
hipError_t launch(const samline::Args &A, uint64_t n, int32_t nmCarryIn, const Buffers &B, hipStream_t st,
                  const samgpu::SortBuffers *S = nullptr);

// The pieces of launch() that the paired encoder (bam_pair_format.hip) runs as well, queued on st.
// nmCarry: nm[i] of n values becomes its own value where that is not kNoNm, else the last such value
// before it, else carryIn (nmTiles: scanTiles(n) entries of scratch).  Instantiated for
// bamline::kNoNm and bampairline::kNoNm.
// checkBlockSizes: *bad += the slots i < n whose block_size is not start[i + 1] - start[i] - 4, inside cap.
template <int32_t kNoNm>
void nmCarry(int32_t *nm, uint64_t n, int32_t *nmTiles, int32_t carryIn, hipStream_t st);
void checkBlockSizes(const uint64_t *start, uint64_t n, const char *out, uint64_t cap, uint32_t *bad, hipStream_t st);

}  // namespace bamgpu
