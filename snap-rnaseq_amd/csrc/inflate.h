// inflate.h -- the device BGZF inflater's kernel (inflate.hip) as fastq_upload.hip launches it.
#pragma once
#include "inflate_block.h"

#include <hip/hip_runtime.h>

namespace inflategpu {

constexpr uint32_t kLdsPerCu = 160u << 10;
// one wave per member in flight, its whole Work in LDS: this many waves fit a CU
constexpr uint32_t kWavesPerCu = kLdsPerCu / (uint32_t)sizeof(inflateblock::Work);
constexpr uint32_t kNoBad = 0xffffffffu;

// Zero bytes the stream buffer carries after the stream: a 64-bit refill at the last member's end
// would stay inside the buffer even if the reader left the member, which it does not.
constexpr uint64_t kInSlack = 64;

// Members 0 .. nMembers of the stream at `in` inflated to out + members[k].outStart, by `waves`
// persistent waves (wave w takes members w, w + waves, ...).  status[k] = the member's
// inflateblock::Status; *firstBad = the lowest k with a status other than ok (kNoBad: none), set to
// kNoBad here.  A refused member writes nothing.
hipError_t launch(const uint8_t *in, const inflateblock::Member *members, uint32_t nMembers, uint8_t *out,
                  uint32_t *status, uint32_t *firstBad, uint32_t waves, hipStream_t st);

}  // namespace inflategpu
