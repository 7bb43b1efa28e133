// bam_passes.h -- the order of the device BAM encoder's passes, stated once for the record rule of
// reads without mate (bam_format.hip) and the pair rule (bam_pair_format.hip): line_passes.h's length
// and write kernels instantiated for the rule, around bam_format.hip's NM carry and block_size check
// and sam_format.hip's sort step and scan.  Device code and its launches: only .hip files include this.
#pragma once
#include "bam_format.h"
#include "line_passes.h"

namespace bamgpu {

// Length pass, NM carry, (sort step,) scan, write pass and the block_size check over n > 0 records of
// rule R, queued on st.  The rule's Side is int32_t: the record's own NM, or kNoNm, after the length
// pass, and the NM it writes after the carry passes, which run over record order whether or not the
// output is sorted.  S non-null: the records in the stable order of R.sortKey.
template <int32_t kNoNm, class Rule>
hipError_t launchRule(const Rule &R, uint64_t n, int32_t nmCarryIn, const Buffers &B, hipStream_t st,
                      const samgpu::SortBuffers *S) {
    using samgpu::KeyOut;
    using samgpu::SlotOrder;
    hipError_t e = S ? samgpu::lengthPass(R, n, B.len, B.nm, B.bad, st, KeyOut<true, Rule>{{}, S->key})
                     : samgpu::lengthPass(R, n, B.len, B.nm, B.bad, st, KeyOut<false, Rule>{});
    if (e != hipSuccess) return e;
    nmCarry<kNoNm>(B.nm, n, B.nmTiles, nmCarryIn, st);
    const uint32_t *len = B.len;
    if (S) {
        if ((e = samgpu::sortStep(*S, B.len, n, st)) != hipSuccess) return e;
        len = S->slotLen;
    }
    samgpu::scanStarts(len, n, B.sums, B.start, st);
    if (S) samgpu::writePass(R, n, B.start, B.nm, B.out, B.outCap, st, SlotOrder<true>{S->order});
    else samgpu::writePass(R, n, B.start, B.nm, B.out, B.outCap, st, SlotOrder<false>{});
    checkBlockSizes(B.start, n, B.out, B.outCap, B.bad, st);
    return hipGetLastError();
}

}  // namespace bamgpu
