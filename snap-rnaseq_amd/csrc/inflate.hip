// inflate.hip -- BGZF members in HBM inflated on the device: bgzf.hip's counterpart.
//
//   bgzf_inflate_kernel   one 64-lane wave (one workgroup) per member in flight; the grid is
//                         persistent, wave w takes members w, w + waves, ...  The member's whole
//                         output (at most 64 KiB), its three code tables and the CRC tables are
//                         the wave's LDS (inflateblock::Work, 69 KiB: two waves per CU).  The
//                         decoder is inflate_block.h's inflateMember() with the wave as its group:
//                         the stream position, the bit buffer (refilled 8 bytes at a time from the
//                         member's bytes in HBM) and the output position are wave-uniform; the
//                         entries of a code's table, the bytes of a match or of a stored block and
//                         the slices of the CRC32 go to the lanes.  A match never reads a byte of
//                         itself (matchSource), so a copy is one step whatever its distance.  An
//                         accepted member is flushed from LDS to its place in the output: single
//                         bytes up to the first 16-byte boundary of the destination, 16-byte
//                         stores, single bytes for the rest.  Each member's status goes to
//                         status[k]; one atomicMin per refused member keeps the lowest index.
#include "inflate.h"

namespace inflategpu {

using namespace inflateblock;

static_assert(kWavesPerCu >= 1, "a member's Work must fit a CU's LDS");

namespace {

struct Wave {
    uint32_t lane;
    template <class F>
    __device__ void forEach(uint32_t n, F fn) const {
        for (uint32_t k = lane; k < n; k += 64) fn(k);
    }
    template <class F>
    __device__ uint32_t serial(F fn) const {
        uint32_t r = 0;
        if (lane == 0) r = fn();
        __syncthreads();
        return __builtin_amdgcn_readfirstlane(r);
    }
    __device__ uint32_t uni(uint32_t x) const { return __builtin_amdgcn_readfirstlane(x); }
    __device__ void sync() const { __syncthreads(); }
    // one unaligned 8-byte load at a wave-uniform address of the member's bytes in HBM.  Staging the
    // compressed bytes in LDS first (4 KiB, reloaded by all lanes) was tried and was slower:
    // 24.6 against 23.4 ms on DESIGN's input
    __device__ uint64_t load64(const uint8_t *p) const {
        uint64_t v;
        __builtin_memcpy(&v, p, 8);
        return (uint64_t)uni((uint32_t)v) | (uint64_t)uni((uint32_t)(v >> 32)) << 32;
    }
    __device__ uint32_t xorAll(uint32_t v) const {
        for (uint32_t o = 32; o; o >>= 1) v ^= __shfl_xor(v, o, 64);
        return v;
    }
    __device__ void copyIn(uint8_t *win, uint32_t pos, const uint8_t *src, uint32_t n) const {
        for (uint32_t k = lane; k < n; k += 64) win[pos + k] = src[k];
    }
    // the bytes before pos were stored by this wave's earlier LDS instructions, which the LDS
    // serves in order; the fence keeps the compiler from moving accesses across the copy
    __device__ void copyMatch(uint8_t *win, uint32_t pos, uint32_t dist, uint32_t n) const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        for (uint32_t k = lane; k < n; k += 64) win[pos + k] = win[pos - dist + matchSource(k, dist)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    __device__ void store(uint8_t *win, uint32_t pos, uint32_t b) const { win[pos] = (uint8_t)b; }
};

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t *__restrict__ in, const Member *__restrict__ members,
                                                          uint32_t nMembers, uint8_t *__restrict__ out,
                                                          uint32_t *__restrict__ status, uint32_t *firstBad) {
    __shared__ Work W;
    const Wave g{threadIdx.x};
    for (uint32_t i = g.lane; i < 256; i += 64) W.crcTab[i] = bgzfblock::crcTableEntry(i);
    if (g.lane < 16) W.xpow[g.lane] = bgzfblock::crcXpow(g.lane);
    for (uint32_t i = g.lane; i < 16; i += 64) W.win[kMaxOut / 4 + i] = 0;
    for (uint32_t k = blockIdx.x; k < nMembers; k += gridDim.x) {
        __syncthreads();
        const Member M = members[k];
        const uint8_t *def = in + M.inStart + M.defOff;
        const uint32_t n = M.inSize - M.defOff - 8;
        uint32_t crcWant = 0;
        for (uint32_t b = 0; b < 4; b++) crcWant |= (uint32_t)def[n + b] << (8 * b);
        const uint32_t st = inflateMember(def, n, M.outSize, g.uni(crcWant), W, g);
        if (g.lane == 0) {
            status[k] = st;
            if (st != kOk) atomicMin(firstBad, k);
        }
        if (st != kOk) continue;
        // the window to out[outStart ..): bytes to the first 16-byte boundary, 16-byte stores, the rest
        __syncthreads();
        uint8_t *dst = out + M.outStart;
        const uint8_t *win = reinterpret_cast<const uint8_t *>(W.win);
        const uint32_t size = M.outSize, toBoundary = (uint32_t)(-(uintptr_t)dst & 15u);
        const uint32_t head = toBoundary < size ? toBoundary : size, nVec = (size - head) / 16;
        if (g.lane < head) dst[g.lane] = win[g.lane];
        for (uint32_t i = g.lane; i < nVec; i += 64) {
            const uint32_t p = head + 16 * i;
            uint4 v;
            v.x = bgzfblock::load32(W.win, p);
            v.y = bgzfblock::load32(W.win, p + 4);
            v.z = bgzfblock::load32(W.win, p + 8);
            v.w = bgzfblock::load32(W.win, p + 12);
            reinterpret_cast<uint4 *>(dst + head)[i] = v;
        }
        for (uint32_t p = head + 16 * nVec + g.lane; p < size; p += 64) dst[p] = win[p];
    }
}

}  // namespace

hipError_t launch(const uint8_t *in, const Member *members, uint32_t nMembers, uint8_t *out, uint32_t *status,
                  uint32_t *firstBad, uint32_t waves, hipStream_t st) {
    hipError_t e = hipMemsetAsync(firstBad, 0xff, 4, st);
    if (e != hipSuccess || nMembers == 0) return e;
    const uint32_t grid = waves < nMembers ? waves : nMembers;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(grid ? grid : 1), dim3(64), 0, st, in, members, nMembers, out, status, firstBad);
    return hipGetLastError();
}

}  // namespace inflategpu
