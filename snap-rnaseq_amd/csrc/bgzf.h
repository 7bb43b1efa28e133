// bgzf.h -- the device BGZF compressor's kernels (bgzf.hip) as output_chain.hip launches them.
#pragma once
#include "bgzf_block.h"

namespace bgzfgpu {

constexpr uint32_t kThreads = 1024;   // one workgroup per block in flight; its LDS leaves room for one per CU

struct Result {
    uint64_t total;     // bytes of the packed stream
    uint32_t nBlocks;
    uint32_t bad;       // members that are not what the size array says (always 0)
};

// Grow-only device buffers for an input of at most capBytes bytes, maxBlocks = blocksOf(capBytes).
struct Buffers {
    uint8_t *slots;     // [maxBlocks * kSlot]  member k at k * kSlot, 16-byte aligned
    uint32_t *sizes;    // [maxBlocks]
    uint64_t *offs;     // [maxBlocks + 1]      member starts in `packed`; offs[nBlocks] = its bytes
    uint32_t *tokens;   // [grid * kBlockIn]    the tokens of the block a workgroup is working on
    uint8_t *packed;    // [maxBlocks * kSlot]
    Result *res;
    uint32_t grid;      // workgroups of the compress pass
};

inline uint64_t blocksOf(uint64_t bytes) { return (bytes + bgzfblock::kBlockIn - 1) / bgzfblock::kBlockIn; }

// Compress pass, scan, gather pass and check over the input bytes at `in` (16-byte aligned), queued
// on st.  The input's size is *nDev when nDev is non-null (a device address that earlier work on st
// writes: the resident records' total) and n otherwise; it is cut at capBytes.  afterCompress /
// afterScan: events recorded between the passes (or null).
hipError_t launch(const uint8_t *in, const uint64_t *nDev, uint64_t n, uint64_t capBytes, const Buffers &B,
                  hipStream_t st, hipEvent_t afterCompress, hipEvent_t afterScan);

}  // namespace bgzfgpu
