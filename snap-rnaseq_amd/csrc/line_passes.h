// line_passes.h -- the length pass and the write pass of the device formatters, stated once and
// instantiated per line rule: single-end SAM (sam_format.hip), paired SAM (sam_pair_format.hip), BAM
// (bam_format.hip) and paired BAM (bam_pair_format.hip).  Device code and its launches: only .hip
// files include this.
//
// A line rule is a small struct passed to the kernels by value.  It carries the rule's arguments
// (samline::Args / PairArgs) and has
//   Fields      what the whole wave reads of a record before lane 0 measures it
//   Side        what the length pass keeps per record for the write pass (samline::Scans, or the NM)
//   SortTables  what sortKey needs beside the fields (rules with a sorted launch)
//   fields(r, g)            every lane of wave g: record r's fields
//   length(F), side(F)      lane 0: the bytes the record takes, and its Side
//   sortKey(tables, F)      lane 0: the record's sort key (rules with a sorted launch)
//   write(r, s, side, g)    every lane of wave g: record r at byte s of the output, through g's window
//                           (side: the whole array, indexed by record)
// The side array is a kernel parameter of its own, not a member of the rule, so that it keeps its
// const __restrict__ in the write kernel and its place in the kernel-argument block.
#pragma once
#include "sam_format.h"
#include "staged_write.h"

namespace samgpu {

// What only the sorted instances of the length and write kernels take, as their last argument: the
// unsorted instances get an empty one, and keep the arguments they had before there was a sorted
// launch (and with them their registers and code).
template <bool Sorted, class Rule>
struct KeyOut {};
template <class Rule>
struct KeyOut<true, Rule> {
    [[no_unique_address]] typename Rule::SortTables tables;   // an empty struct takes no argument bytes
    uint32_t *key;   // [n] out: Rule::sortKey per record
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

// One wave per record: len[r] = its bytes, side[r], and (Sorted) key[r] = its sort key.
template <class Rule, bool Sorted>
__global__ __launch_bounds__(256) void line_length_kernel(Rule R, uint64_t n, uint32_t *__restrict__ len,
                                                          typename Rule::Side *__restrict__ side, KeyOut<Sorted, Rule> K) {
    const Wave g{nullptr, 0, 0, threadIdx.x & 63u};
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + threadIdx.x / 64u; r < n; r += waves) {
        const typename Rule::Fields F = R.fields(r, g);
        if (g.lane == 0) {
            len[r] = R.length(F);
            side[r] = R.side(F);
            if constexpr (Sorted) K.key[r] = R.sortKey(K.tables, F);
        }
    }
}

// One workgroup per kRecsPerGroup consecutive slots, staged through an LDS window of kTileBytes
// (staged_write.h).  Sorted: start[] is over output slots and slot j holds record O.order[j] (the
// side array stays per record), else slot j holds record j.
template <class Rule, bool Sorted>
__global__ __launch_bounds__(256) void line_write_kernel(Rule R, uint64_t n, const uint64_t *__restrict__ start,
                                                         const typename Rule::Side *__restrict__ side,
                                                         char *__restrict__ out, uint64_t cap, SlotOrder<Sorted> O) {
    __shared__ uint4 tile[kTileBytes / 16];
    const uint64_t first = (uint64_t)blockIdx.x * kRecsPerGroup;
    const uint64_t end = first + kRecsPerGroup < n ? first + kRecsPerGroup : n;
    staged::Windows<kTileBytes> W(start, first, end);
    if (W.r1 > cap) return;   // the host's bound on the output was too small: the check kernel reports it
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    for (; W.more(); W.flush(out, tile)) {
        const Wave g{reinterpret_cast<char *>(tile), W.w0, W.w1(), lane};
        for (uint64_t j = first + wave; j < end; j += 4) {
            const uint64_t s = start[j], e = start[j + 1];
            if (!W.holds(s, e)) continue;
            const uint64_t r = O.record(j);
            if (Sorted && r >= n) continue;   // not a record (never): the slot is empty, the check reports it
            R.write(r, s, side, g);
        }
    }
}

// The grid of a kernel with one lane per item.
inline dim3 perItem(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// Clear *bad (what the check kernel after the write pass counts into) and queue the length pass over
// n > 0 records on st: four waves a workgroup, the waves striding over the records.
template <class Rule, bool Sorted>
hipError_t lengthPass(const Rule &R, uint64_t n, uint32_t *len, typename Rule::Side *side, uint32_t *bad, hipStream_t st,
                      KeyOut<Sorted, Rule> K) {
    const hipError_t e = hipMemsetAsync(bad, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint64_t blocks = (n + 3) / 4 < 65536 ? (n + 3) / 4 : 65536;
    hipLaunchKernelGGL((line_length_kernel<Rule, Sorted>), dim3((unsigned)blocks), dim3(256), 0, st, R, n, len, side, K);
    return hipSuccess;
}

// Queue the write pass over n > 0 slots on st.
template <class Rule, bool Sorted>
void writePass(const Rule &R, uint64_t n, const uint64_t *start, const typename Rule::Side *side, char *out, uint64_t cap,
               hipStream_t st, SlotOrder<Sorted> O) {
    const uint64_t groups = (n + kRecsPerGroup - 1) / kRecsPerGroup;
    hipLaunchKernelGGL((line_write_kernel<Rule, Sorted>), dim3((unsigned)groups), dim3(256), 0, st, R, n, start, side, out, cap, O);
}

}  // namespace samgpu
