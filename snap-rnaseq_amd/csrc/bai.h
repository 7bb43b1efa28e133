// bai.h -- the device BAI builder's kernels (bai.hip) as output_chain.hip launches them.
#pragma once
#include "bai_index.h"

#include <hip/hip_runtime.h>

namespace baigpu {

constexpr uint32_t kThreads = 256;      // per-record, per-chunk and write kernels
constexpr uint32_t kScanThreads = 1024; // the per-reference scans and the linear index's back-fill
constexpr int kPasses = 7;              // fields, chunk heads, sort, counts, linear index, layout + write, check

struct Result {
    uint64_t total;        // bytes of the index
    uint64_t linTotal;     // intervals of all references
    uint32_t bad;          // refused or unsorted records, counts that do not add up (always 0)
    uint32_t nChunks, nBins;
    uint32_t noCoorFirst;  // the first record without a reference (n: none)
};

// What the passes keep of one reference.
struct RefInfo {
    uint32_t first, last;            // its records
    uint32_t mapped, unmapped;
    int32_t maxEnd;
    uint32_t chunkFirst, chunkEnd;   // its chunks in sorted order
    uint32_t binFirst, binEnd;       // its bins among all bin heads
    uint32_t pad;
};

// One device allocation carved up for n records over nRef references (all offsets 16-byte aligned).
struct Layout {
    uint64_t ref, bin, beg, end, vbeg, vend, head, tail, headIdx;       // per record (head, headIdx: n + 1)
    uint64_t key, keySorted, val, valSorted, cbeg, cend, binHead, binIdx, binStart;   // per chunk (n, n + 1)
    uint64_t info, refOff, linBase;                                     // per reference (nRef, nRef + 1)
    uint64_t lin, temp, res;
    uint64_t linCap, tempBytes, bytes;
};

// rocPRIM's temporary storage for the scans and the sort over n records.
hipError_t tempBytes(uint64_t n, hipStream_t st, uint64_t *bytes);
Layout layout(uint64_t n, uint64_t nRef, uint64_t tempBytes);

// All passes over the n records at text + start[i] (start[n]: their bytes), queued on st.  coff: the
// device compressor's member offsets (bgzfgpu::Buffers::offs).  The index goes to out (outCap >=
// baiindex::sizeBound, 4-byte aligned), its size and the checks to the Result at work + L.res.
// ev: kPasses + 1 events recorded around the passes, or null.
hipError_t launch(const uint8_t *text, const uint64_t *start, uint64_t n, uint32_t nRef, const uint64_t *coff,
                  uint64_t streamOffset, char *work, const Layout &L, uint8_t *out, uint64_t outCap, hipStream_t st,
                  hipEvent_t *ev);

}  // namespace baigpu
