// fastq_parse.hip -- FASTQ text in device memory to a resident read batch (gfx950, wave64):
//   1. fastq_count_kernel    '\n' bytes per tile of kTileBytes (SWAR compare, popcount, reduction)
//   2. samgpu::scanStarts    the tiles' first newline ranks (fastq_upload.hip queues it)
//   3. fastq_lines_kernel    each tile rescans and stores its newline positions at their ranks
//   4. fastq_record_kernel   fastq_record.h per record, a wave per record: trimmed line bounds, the
//                            three lengths, Read::clip, the first record without '@' header (an
//                            atomicMin per wave)
//   4b. fastq_limits_kernel  the longest unclipped read and the longest id of the batch (a wave
//                            reduction, then one atomicMax each per wave)
//   5. samgpu::scanStarts    64-bit starts of the records' bases and ids
//   6. fastq_pack_kernel     ids, bases and qualities to their places, staged through LDS so that
//                            the stores are whole 16-byte chunks (staged_write.h, once per output)
// All byte offsets are 64-bit.  The text buffer is fqgpu::textCapacity(nBytes) long and zero from
// nBytes on, so the newline passes load whole 64-byte lane spans without a tail case.
#include "fastq_parse.h"

#include "staged_write.h"

namespace fqgpu {
namespace {

// bit k of the result: byte k of w is '\n'
__device__ inline uint32_t newlineNibble(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 where a byte of x is 0
    return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;
}

// bit k: text[off + k] is '\n', k < 64 (off a multiple of 64 inside the buffer)
__device__ inline uint64_t newlineMask(const char *__restrict__ text, uint64_t off) {
    const uint4 *p = reinterpret_cast<const uint4 *>(text + off);
    uint64_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint4 v = p[j];
        const uint32_t h = newlineNibble(v.x) | newlineNibble(v.y) << 4 | newlineNibble(v.z) << 8 | newlineNibble(v.w) << 12;
        m |= (uint64_t)h << (16 * j);
    }
    return m;
}

__global__ __launch_bounds__(256) void fastq_count_kernel(const char *__restrict__ text, uint64_t nBytes,
                                                          uint32_t *__restrict__ counts) {
    __shared__ uint32_t sh[4];
    const uint64_t off = (uint64_t)blockIdx.x * kTileBytes + threadIdx.x * 64ull;
    uint32_t c = off < nBytes ? (uint32_t)__popcll(newlineMask(text, off)) : 0u;
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x / 64u] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void fastq_lines_kernel(const char *__restrict__ text, uint64_t nBytes,
                                                          const uint64_t *__restrict__ tileStart,
                                                          uint64_t *__restrict__ nl, uint64_t nNl) {
    __shared__ uint32_t sh[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    const uint64_t off = (uint64_t)blockIdx.x * kTileBytes + threadIdx.x * 64ull;
    uint64_t m = off < nBytes ? newlineMask(text, off) : 0ull;
    const uint32_t c = (uint32_t)__popcll(m);
    uint32_t incl = c;   // inclusive scan over the wave
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += t;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint32_t before = incl - c;
    for (uint32_t w = 0; w < wave; w++) before += sh[w];
    uint64_t rank = tileStart[blockIdx.x] + before;
    while (m) {
        const uint32_t k = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        if (rank < nNl) nl[rank] = off + k;
        rank++;
        m &= m - 1;
    }
}

// A 64-lane wave as fastq_record.h's group.
struct Wave {
    uint32_t lane;
    template <class P>
    __device__ uint64_t firstOf(uint64_t n, P p) const {
        for (uint64_t base = 0; base < n; base += 64) {
            const uint64_t k = base + lane;
            const bool hit = k < n && p(k);
            const unsigned long long m = __ballot(hit);
            if (m) return base + (uint64_t)__ffsll(m) - 1;
        }
        return n;
    }
    __device__ uint64_t firstByte(const char *p, uint64_t n, char c) const {
        return firstOf(n, [=](uint64_t k) { return p[k] == c; });
    }
};

struct Lines {
    const uint64_t *nl;
    uint64_t nNl, nBytes;
    __device__ uint64_t start(uint64_t i) const { return i ? nl[i - 1] + 1 : 0ull; }
    __device__ uint64_t end(uint64_t i) const { return i < nNl ? nl[i] : nBytes; }
};

__global__ __launch_bounds__(256) void fastq_record_kernel(const char *__restrict__ text, Lines L, uint64_t n,
                                                           int clipping, Records R, Totals *tot) {
    const Wave g{threadIdx.x & 63u};
    const uint64_t nWaves = (uint64_t)gridDim.x * 4u;
    // the wave's share of the totals, added once at the end: an atomic per record on the one address
    // was the whole pass (12 ms of 12.8 per 1M reads)
    unsigned long long baseBytes = 0, firstBad = ~0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + threadIdx.x / 64u; r < n; r += nWaves) {
        const fastqrec::Record F = fastqrec::record(
            text, r, [=](uint64_t i) { return L.start(i); }, [=](uint64_t i) { return L.end(i); }, g);
        uint32_t front = 0, len = 0;
        if (!F.bad) {
            const char *q = text + F.qualAt;
            const uint32_t nq = F.qualLen;
            fastqrec::clip([=](uint64_t k) { return k < nq ? q[k] : (char)0; }, F.baseLen, clipping, front, len, g);
        }
        if (g.lane == 0) {
            R.idLen[r] = F.bad ? 0u : F.idLen;
            R.baseLen[r] = F.bad ? 0u : F.baseLen;
            R.qualLen[r] = F.bad ? 0u : F.qualLen;
            R.front[r] = front;
            R.clipLen[r] = len;
        }
        if (F.bad) firstBad = firstBad < r ? firstBad : r;
        else baseBytes += F.baseLen;
    }
    if (g.lane == 0) {
        if (firstBad != ~0ull) atomicMin(&tot->firstBad, firstBad);
        if (baseBytes) atomicAdd(&tot->baseBytes, baseBytes);
    }
}

// Maxima of the two length arrays: grid-stride over the records, a wave reduction, one atomic per
// wave and array (a single-address atomic per record is what the record pass avoids).
__global__ __launch_bounds__(256) void fastq_limits_kernel(const uint32_t *__restrict__ baseLen,
                                                           const uint32_t *__restrict__ idLen, uint64_t n, Totals *tot) {
    uint32_t mb = 0, mi = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n; r += stride) {
        const uint32_t b = baseLen[r], i = idLen[r];
        mb = mb > b ? mb : b;
        mi = mi > i ? mi : i;
    }
    for (int o = 32; o; o >>= 1) {
        const uint32_t b = __shfl_xor(mb, o), i = __shfl_xor(mi, o);
        mb = mb > b ? mb : b;
        mi = mi > i ? mi : i;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (mb) atomicMax(&tot->maxBaseLen, mb);
        if (mi) atomicMax(&tot->maxIdLen, mi);
    }
}

// One output of the copy pass over the group's records [first, end): record j's piece is src[j]'s
// first `valid` bytes, then 0x00, start[j + 1] - start[j] bytes in all, at out + start[j], staged
// through windows of kStageBytes in LDS and stored as whole uint4 chunks (staged_write.h).
template <class Src>
__device__ void packStream(char *__restrict__ out, const uint64_t *__restrict__ start, uint64_t first, uint64_t end,
                           uint4 *tile, Src src) {
    char *lds = reinterpret_cast<char *>(tile);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    for (staged::Windows<kStageBytes> W(start, first, end); W.more(); W.flush(out, tile)) {
        const uint64_t w0 = W.w0, w1 = W.w1();
        for (uint64_t j = first + wave; j < end; j += 4) {
            const uint64_t s = start[j], e = start[j + 1];
            if (!W.holds(s, e)) continue;
            const char *p;
            uint32_t valid;
            src(j, p, valid);
            const uint64_t lo = s > w0 ? s : w0, hi = e < w1 ? e : w1;
            for (uint64_t at = lo + lane; at < hi; at += 64) {
                const uint64_t k = at - s;
                lds[at - w0] = k < valid ? p[k] : (char)0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void fastq_pack_kernel(const char *__restrict__ text, Lines L, uint64_t n, Records R,
                                                         const uint64_t *__restrict__ baseStart,
                                                         const uint64_t *__restrict__ idStart, char *__restrict__ bases,
                                                         char *__restrict__ quals, char *__restrict__ ids,
                                                         uint64_t *__restrict__ offsets, uint32_t *__restrict__ lengths) {
    __shared__ uint4 tile[kStageBytes / 16];
    const uint64_t first = (uint64_t)blockIdx.x * kRecsPerGroup;
    const uint64_t end = first + kRecsPerGroup < n ? first + kRecsPerGroup : n;
    if (first + threadIdx.x < end) {
        const uint64_t j = first + threadIdx.x;
        offsets[j] = baseStart[j] + R.front[j];
        lengths[j] = R.clipLen[j];
    }
    packStream(ids, idStart, first, end, tile, [=](uint64_t j, const char *&p, uint32_t &valid) {
        p = text + L.start(4 * j) + 1;
        valid = R.idLen[j];
    });
    packStream(bases, baseStart, first, end, tile, [=](uint64_t j, const char *&p, uint32_t &valid) {
        p = text + L.start(4 * j + 1);
        valid = R.baseLen[j];
    });
    packStream(quals, baseStart, first, end, tile, [=](uint64_t j, const char *&p, uint32_t &valid) {
        p = text + L.start(4 * j + 3);
        valid = R.qualLen[j] < R.baseLen[j] ? R.qualLen[j] : R.baseLen[j];
    });
}

}  // namespace

void countNewlines(const char *text, uint64_t nBytes, uint32_t *counts, hipStream_t st) {
    hipLaunchKernelGGL(fastq_count_kernel, dim3((unsigned)tiles(nBytes)), dim3(256), 0, st, text, nBytes, counts);
}

void lineStarts(const char *text, uint64_t nBytes, const uint64_t *tileStart, uint64_t *nl, uint64_t nNl, hipStream_t st) {
    hipLaunchKernelGGL(fastq_lines_kernel, dim3((unsigned)tiles(nBytes)), dim3(256), 0, st, text, nBytes, tileStart, nl, nNl);
}

void records(const char *text, uint64_t nBytes, const uint64_t *nl, uint64_t nNl, uint64_t n, int clipping,
             const Records &R, Totals *tot, hipStream_t st) {
    // 2048 workgroups of four waves fill the device at 8 waves per SIMD; the waves stride over the records
    const uint64_t blocks = (n + 3) / 4 < 2048 ? (n + 3) / 4 : 2048;
    hipLaunchKernelGGL(fastq_record_kernel, dim3((unsigned)blocks), dim3(256), 0, st, text, Lines{nl, nNl, nBytes}, n,
                       clipping, R, tot);
}

void limits(const uint32_t *baseLen, const uint32_t *idLen, uint64_t n, Totals *tot, hipStream_t st) {
    // 16 records per lane until 256 workgroups (one per CU) are reached: 1,024 atomics per array at the most
    const uint64_t blocks = (n + 4095) / 4096 < 256 ? (n + 4095) / 4096 : 256;
    hipLaunchKernelGGL(fastq_limits_kernel, dim3((unsigned)blocks), dim3(256), 0, st, baseLen, idLen, n, tot);
}

void pack(const char *text, uint64_t nBytes, const uint64_t *nl, uint64_t nNl, uint64_t n, const Records &R,
          const uint64_t *baseStart, const uint64_t *idStart, char *bases, char *quals, char *ids,
          uint64_t *offsets, uint32_t *lengths, hipStream_t st) {
    const uint64_t groups = (n + kRecsPerGroup - 1) / kRecsPerGroup;
    hipLaunchKernelGGL(fastq_pack_kernel, dim3((unsigned)groups), dim3(256), 0, st, text, Lines{nl, nNl, nBytes}, n, R,
                       baseStart, idStart, bases, quals, ids, offsets, lengths);
}

}  // namespace fqgpu
