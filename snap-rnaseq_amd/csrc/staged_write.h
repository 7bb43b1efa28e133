// staged_write.h -- the LDS-staged write of a workgroup's records into one contiguous byte range of
// an output in HBM: the window arithmetic and the flush, stated once.  The write pass of the SAM,
// paired SAM and BAM formatters (line_passes.h) and the FASTQ copy pass (fastq_parse.hip) use it;
// what they differ in is how a wave composes a record into the window.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace staged {

// One workgroup of 256 lanes writes the records [first, end): record j is the bytes [start[j],
// start[j + 1]) of `out`, so the group owns [r0, r1) = [start[first], start[end)) and stores nothing
// outside it.  The range is taken in windows [w0, w1()) of TileBytes that are 16-byte aligned in the
// output (an LDS chunk is then a 16-byte aligned store; `out` is 16-byte aligned):
//     for (staged::Windows<TileBytes> W(start, first, end); W.more(); W.flush(out, tile))
//         for (uint64_t j = first + wave; j < end; j += 4)      // wave = threadIdx.x / 64
//             if (W.holds(start[j], start[j + 1])) <the wave puts record j's bytes that fall into
//                                                   the window at tile[at - W.w0]>
// A record longer than a window comes round once per window.  The composer stays in the caller's
// loop and is not handed in as a functor: a closure passed into a device function changed the code
// of the formatters' composers (profiles/r23/README.md).  Every lane of the workgroup runs the loop,
// with the same first and end; tile: TileBytes of LDS.
template <uint32_t TileBytes>
struct Windows {
    uint64_t r0, r1, w0;
    __device__ Windows(const uint64_t *__restrict__ start, uint64_t first, uint64_t end)
        : r0(start[first]), r1(start[end]), w0(r0 & ~15ull) {}
    __device__ bool more() const { return w0 < r1; }
    __device__ uint64_t w1() const { return w0 + TileBytes < r1 ? w0 + TileBytes : r1; }
    __device__ bool holds(uint64_t s, uint64_t e) const { return !(e <= w0 || s >= w1()); }
    // The window is composed: store it and go to the next one.  Whole uint4 chunks where all 16
    // bytes are the group's, bytewise at its two ragged ends (the neighbouring groups own the rest of
    // those chunks).  The first __syncthreads() waits for the composers, the second frees the tile.
    __device__ void flush(char *__restrict__ out, const uint4 *tile) {
        const char *lds = reinterpret_cast<const char *>(tile);
        __syncthreads();
        const uint32_t chunks = (uint32_t)((w1() - w0 + 15) / 16);
        for (uint32_t c = threadIdx.x; c < chunks; c += 256) {
            const uint64_t a = w0 + 16ull * c;
            if (a >= r0 && a + 16 <= r1) {
                *reinterpret_cast<uint4 *>(out + a) = tile[c];
            } else {
                const uint64_t lo = a > r0 ? a : r0, hi = a + 16 < r1 ? a + 16 : r1;
                for (uint64_t b = lo; b < hi; b++) out[b] = lds[b - w0];
            }
        }
        __syncthreads();
        w0 += TileBytes;
    }
};

}  // namespace staged
