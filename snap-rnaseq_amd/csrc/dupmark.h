// dupmark.h -- the device duplicate marking's kernels (dupmark.hip) as output_chain.hip launches them.
#pragma once
#include "dupmark_rule.h"

#include <hip/hip_runtime.h>

namespace dupgpu {

constexpr uint32_t kThreads = 256;     // every kernel's workgroup
constexpr uint32_t kLanes = 8;         // the lanes that share one record's QUAL in the score pass
constexpr uint32_t kScoreRecords = kThreads / kLanes;   // records of one workgroup of the score pass: 32
constexpr int kPasses = 5;             // fields + score, run numbering, best per group, mark, check

struct Result {
    unsigned long long marked;     // records the mark pass set 0x400 on
    unsigned long long expected;   // the sum over groups of size - 1
    unsigned long long groups;     // groups of two or more
    uint32_t refused;              // truncated, refused by bai_index.h, l_seq > 2^24, out of order (always 0)
    uint32_t mates;                // records with FLAG 0x1 (always 0)
};

// One device allocation carved up for n records (all offsets 16-byte aligned).
struct Layout {
    uint64_t score, info, head, runIdx;   // per record (head, runIdx: n + 1)
    uint64_t best, size;                  // per (run, strand): 2 n
    uint64_t temp, res;
    uint64_t tempBytes, bytes;
};

// rocPRIM's temporary storage for the scan over n records.
hipError_t tempBytes(uint64_t n, hipStream_t st, uint64_t *bytes);
Layout layout(uint64_t n, uint64_t tempBytes);

// All passes over the n records at text + start[i] (start[n]: their bytes), queued on st: byte 19 of
// every accepted record is rewritten in place, the counts go to the Result at work + L.res.
// ev: kPasses + 1 events recorded around the passes, or null.
hipError_t launch(uint8_t *text, const uint64_t *start, uint64_t n, uint32_t nRef, char *work, const Layout &L,
                  hipStream_t st, hipEvent_t *ev);

}  // namespace dupgpu
