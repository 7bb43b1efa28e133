// bgzf.hip -- BGZF members of bytes in HBM, written on the device.
//
//   compress  one workgroup of 1024 lanes per block of 0xff00 input bytes (workgroups take blocks
//             k, k + grid, ...).  The block, the hash table, one chunk's match arrays, the histograms
//             and the code tables live in LDS (133 KB: one workgroup per CU, 16 waves).  The steps are
//             bgzf_block.h's: table windows (read, barrier, atomicMax, barrier), bestMatch for every
//             position of a chunk, the greedy parse marked by pointer jumping, tokens compacted into
//             a per-workgroup HBM scratch through a workgroup scan, histograms by LDS atomics; then
//             one lane makes the code lengths (the sort is a parallel rank), and the token bits are
//             placed by a workgroup scan and OR-ed into the member, which is built in the LDS words
//             the block no longer needs and flushed with 16-byte stores into the member's slot
//   scan      one workgroup: exclusive scan of the member sizes
//   gather    one workgroup per member: slot -> its place in the packed stream
//   check     per member: BSIZE, ISIZE and its extent must be what the size array says
#include "bgzf.h"

namespace bgzfgpu {

using namespace bgzfblock;

namespace {

constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kPerLane = kChunk / kThreads;   // chunk positions per lane
constexpr uint32_t kJumpRounds = 12;               // 2^12 hops pass a chunk of kChunk positions
static_assert(kChunk == 1u << kJumpRounds && kChunk % kThreads == 0 && kWindow <= kThreads, "chunk / window split");
static_assert(kCrcSlice * kThreads >= kBlockIn, "one CRC slice per lane");

struct Lds {
    uint32_t data[kDataWords];   // the block; later the member under construction
    uint32_t table[kTable];      // hash -> largest position + 1 of the windows so far
    uint16_t len[kChunk], dist[kChunk], jump[kChunk];
    uint8_t mark[kChunk];        // the greedy parse stops here
    uint32_t litFreq[kLitPad], distFreq[kDistPad];
    uint16_t sortedLit[kLitPad];
    Plan plan;
    Scratch scratch;
    uint32_t crcTab[256], xpow[16];
    uint32_t waveTot[kWaves];
    uint32_t entry;              // where the parse enters the next chunk
    uint32_t usedLit, crc, dyn, size;
};

struct AtomicOr {   // many writers
    uint32_t *words;
    __device__ void orWord(uint32_t i, uint32_t x) {
        if (i < kDataWords) atomicOr(&words[i], x);
    }
};

// exclusive scan of v over the workgroup's lanes; total: the sum.  Two barriers.
__device__ uint32_t scanLanes(uint32_t v, uint32_t *waveTot, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    uint32_t inc = v;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) waveTot[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kWaves; w++) {
        const uint32_t x = waveTot[w];
        before += w < wave ? x : 0u;
        all += x;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// the input's size: the device value where there is one, cut at capBytes
__device__ uint64_t inputBytes(const uint64_t *nDev, uint64_t n, uint64_t capBytes) {
    const uint64_t v = nDev ? *nDev : n;
    return v < capBytes ? v : capBytes;
}

__global__ __launch_bounds__(kThreads) void bgzf_compress_kernel(const uint8_t *__restrict__ in, const uint64_t *nDev,
                                                                 uint64_t nHost, uint64_t capBytes,
                                                                 uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                                 uint32_t *__restrict__ tokens, Result *res) {
    __shared__ Lds L;
    const uint32_t t = threadIdx.x;
    const uint64_t n = inputBytes(nDev, nHost, capBytes);
    const uint64_t nBlocks = (n + kBlockIn - 1) / kBlockIn;
    uint32_t *tok = tokens + (uint64_t)blockIdx.x * kBlockIn;
    if (t < 256) L.crcTab[t] = crcTableEntry(t);
    else if (t < 256 + 16) L.xpow[t - 256] = crcXpow(t - 256);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(L.data);
    for (uint64_t k = blockIdx.x; k < nBlocks; k += gridDim.x) {
        __syncthreads();
        const uint32_t m = (uint32_t)(n - k * kBlockIn < kBlockIn ? n - k * kBlockIn : kBlockIn);
        const uint8_t *src = in + k * kBlockIn;
        const uint32_t nVec = m / 16;
        for (uint32_t i = t; i < nVec; i += kThreads)
            reinterpret_cast<uint4 *>(L.data)[i] = reinterpret_cast<const uint4 *>(src)[i];
        for (uint32_t i = nVec * 4 + t; i < kDataWords; i += kThreads) L.data[i] = 0;
        for (uint32_t i = t; i < kTable; i += kThreads) L.table[i] = 0;
        if (t < kLitPad) L.litFreq[t] = 0;
        if (t < kDistPad) L.distFreq[t] = 0;
        if (t == 0) {
            L.entry = 0;
            L.usedLit = 0;
            L.crc = 0;
        }
        __syncthreads();
        for (uint32_t i = nVec * 16 + t; i < m; i += kThreads) bytes[i] = src[i];
        __syncthreads();
        if (kCrcSlice * t < m) {
            const uint32_t p = kCrcSlice * t, len = m - p < kCrcSlice ? m - p : kCrcSlice;
            atomicXor(&L.crc, crcAdvance(crcSlice(L.crcTab, L.data, p, len), m - p - len, L.xpow));
        }
        uint32_t nTok = 0;
        for (uint32_t c0 = 0; c0 < m; c0 += kChunk) {
            const uint32_t end = c0 + kChunk < m ? c0 + kChunk : m;
            // find: the table's candidates, window by window
            for (uint32_t w0 = c0; w0 < end; w0 += kWindow) {
                const uint32_t p = w0 + t;
                const bool mine = t < kWindow && p + 4 <= m;
                uint32_t h = 0;
                if (mine) {
                    h = hash4(load32(L.data, p));
                    const uint32_t c = L.table[h];
                    L.dist[p - c0] = (uint16_t)(c ? c - 1 : kNoCand);
                }
                __syncthreads();
                if (mine) atomicMax(&L.table[h], p + 1);
                __syncthreads();
            }
            // every position's match, and where the parse would go from it
            const uint32_t entry = L.entry;
            for (uint32_t i = 0; i < kPerLane; i++) {
                const uint32_t rel = t + kThreads * i, p = c0 + rel;
                if (p < end) {
                    uint32_t len, dist;
                    bestMatch(L.data, p, m, L.dist[rel], len, dist);
                    L.len[rel] = (uint16_t)len;
                    L.dist[rel] = (uint16_t)dist;
                    L.jump[rel] = (uint16_t)(p + (len ? len : 1u));
                    L.mark[rel] = p == entry;
                }
            }
            __syncthreads();
            // parse: after round r the marks cover 2^(r + 1) - 1 hops from the entry, jump is 2^(r + 1) hops
            for (uint32_t round = 0; round < kJumpRounds; round++) {
                uint32_t j[kPerLane], jj[kPerLane];
                bool mk[kPerLane];
                for (uint32_t i = 0; i < kPerLane; i++) {
                    const uint32_t rel = t + kThreads * i;
                    j[i] = jj[i] = end;
                    mk[i] = false;
                    if (c0 + rel < end) {
                        j[i] = L.jump[rel];
                        mk[i] = L.mark[rel] != 0;
                        jj[i] = j[i] < end ? L.jump[j[i] - c0] : j[i];
                    }
                }
                __syncthreads();
                for (uint32_t i = 0; i < kPerLane; i++) {
                    const uint32_t rel = t + kThreads * i;
                    if (c0 + rel < end) {
                        L.jump[rel] = (uint16_t)jj[i];
                        if (mk[i] && j[i] < end) L.mark[j[i] - c0] = 1;
                    }
                }
                __syncthreads();
            }
            // tokens of the marked positions, in order: lane t owns kPerLane consecutive positions
            uint32_t cnt = 0;
            for (uint32_t i = 0; i < kPerLane; i++) {
                const uint32_t rel = kPerLane * t + i;
                cnt += c0 + rel < end && L.mark[rel];
            }
            uint32_t total;
            uint32_t at = nTok + scanLanes(cnt, L.waveTot, total);
            for (uint32_t i = 0; i < kPerLane; i++) {
                const uint32_t rel = kPerLane * t + i, p = c0 + rel;
                if (p >= end || !L.mark[rel]) continue;
                const uint32_t len = L.len[rel];
                if (len) {
                    const uint32_t dist = L.dist[rel];
                    uint32_t sym, eb, ev;
                    lenSym(len, sym, eb, ev);
                    atomicAdd(&L.litFreq[sym], 1u);
                    distSym(dist, sym, eb, ev);
                    atomicAdd(&L.distFreq[sym], 1u);
                    tok[at++] = matchToken(len, dist);
                } else {
                    const uint32_t b = byteAt(L.data, p);
                    atomicAdd(&L.litFreq[b], 1u);
                    tok[at++] = b;
                }
                if (p + (len ? len : 1u) >= end) L.entry = p + (len ? len : 1u);   // one position leaves the chunk
            }
            nTok += total;
            __syncthreads();
        }
        if (t == 0) L.litFreq[kEob] = 1;
        __syncthreads();
        if (t < kLit && L.litFreq[t]) {
            L.sortedLit[rankOf(L.litFreq, kLit, t)] = (uint16_t)t;
            atomicAdd(&L.usedLit, 1u);
        }
        __syncthreads();
        if (t == 0) {
            makePlan(L.litFreq, L.distFreq, L.sortedLit, L.usedLit, L.plan, L.scratch);
            const uint32_t dynBytes = (L.plan.dynBits + 7) / 8;
            L.dyn = dynBytes <= 5 + m;
            L.size = 18 + (L.dyn ? dynBytes : 5 + m) + 8;
            sizes[k] = L.size;
        }
        __syncthreads();
        const uint32_t size = L.size;
        uint8_t *out = slots + k * kSlot;
        if (L.dyn) {
            for (uint32_t i = t; i < kDataWords; i += kThreads) L.data[i] = 0;
            __syncthreads();
            uint32_t bit = kDeflateBit;
            if (t == 0) {
                PlainOr o{L.data};
                writeGzipHeader(o, size);
                L.entry = writeDynamicHeader(o, kDeflateBit, L.plan);
            }
            __syncthreads();
            bit = L.entry;
            for (uint32_t b0 = 0; b0 < nTok; b0 += kThreads) {
                uint64_t bits = 0;
                uint32_t nb = 0;
                if (b0 + t < nTok) tokenBits(tok[b0 + t], L.plan, bits, nb);
                uint32_t total;
                const uint32_t off = scanLanes(nb, L.waveTot, total);
                AtomicOr o{L.data};
                orBits(o, bit + off, bits, nb);
                bit += total;
            }
            __syncthreads();
            if (t == 0) {
                PlainOr o{L.data};
                orBits(o, bit, L.plan.litCode[kEob], L.plan.litLen[kEob]);
                if (bit + L.plan.litLen[kEob] != kDeflateBit + L.plan.dynBits) atomicAdd(&res->bad, 1u);
                orBits(o, (size - 8) * 8, L.crc, 32);
                orBits(o, (size - 4) * 8, m, 32);
            }
            __syncthreads();
            const uint32_t nOut = (size + 15) / 16;
            for (uint32_t i = t; i < nOut; i += kThreads)
                reinterpret_cast<uint4 *>(out)[i] = reinterpret_cast<const uint4 *>(L.data)[i];
        } else {
            if (t < 32) {   // the 18 + 5 bytes before the stored bytes, the 8 after them
                uint32_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                PlainOr o{head};
                writeGzipHeader(o, size);
                orBits(o, kDeflateBit, 1u | (uint64_t)m << 8 | (uint64_t)(~m & 0xffffu) << 24, 40);
                const uint32_t tail[2] = {L.crc, m};
                if (t < 23) out[t] = (uint8_t)(head[t >> 2] >> ((t & 3u) * 8u));
                else if (t < 31) out[size - 8 + (t - 23)] = (uint8_t)(tail[(t - 23) >> 2] >> (((t - 23) & 3u) * 8u));
            }
            for (uint32_t i = t; i < m; i += kThreads) out[23 + i] = bytes[i];
        }
    }
}

__global__ __launch_bounds__(kThreads) void bgzf_scan_kernel(const uint64_t *nDev, uint64_t nHost, uint64_t capBytes,
                                                             const uint32_t *__restrict__ sizes, uint64_t *__restrict__ offs,
                                                             Result *res) {
    __shared__ uint32_t waveTot[kWaves];
    const uint64_t nBlocks = (inputBytes(nDev, nHost, capBytes) + kBlockIn - 1) / kBlockIn;
    uint64_t running = 0;
    for (uint64_t b0 = 0; b0 < nBlocks; b0 += kThreads) {
        const uint64_t i = b0 + threadIdx.x;
        const uint32_t v = i < nBlocks ? sizes[i] : 0u;
        uint32_t total;
        const uint32_t before = scanLanes(v, waveTot, total);
        if (i < nBlocks) offs[i] = running + before;
        running += total;
    }
    if (threadIdx.x == 0) {
        offs[nBlocks] = running;
        res->total = running;
        res->nBlocks = (uint32_t)nBlocks;
    }
}

__global__ __launch_bounds__(256) void bgzf_gather_kernel(const uint64_t *nDev, uint64_t nHost, uint64_t capBytes,
                                                          const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                          const uint64_t *__restrict__ offs, uint8_t *__restrict__ packed) {
    const uint64_t nBlocks = (inputBytes(nDev, nHost, capBytes) + kBlockIn - 1) / kBlockIn;
    const uint64_t k = blockIdx.x;
    if (k >= nBlocks) return;
    const uint8_t *src = slots + k * kSlot;
    const uint32_t size = sizes[k] < kSlot ? sizes[k] : kSlot;
    uint8_t *dst = packed + offs[k];
    // bytes up to the first 4-byte boundary of the packed stream, whole words, the rest
    const uint32_t head = (uint32_t)(-(uintptr_t)dst & 3u) < size ? (uint32_t)(-(uintptr_t)dst & 3u) : size;
    const uint32_t words = (size - head) / 4;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < words; i += 256) {
        const uint32_t p = head + 4 * i;
        reinterpret_cast<uint32_t *>(dst + head)[i] =
            (uint32_t)src[p] | (uint32_t)src[p + 1] << 8 | (uint32_t)src[p + 2] << 16 | (uint32_t)src[p + 3] << 24;
    }
    for (uint32_t p = head + 4 * words + threadIdx.x; p < size; p += 256) dst[p] = src[p];
}

// member k of the packed stream: the gzip magic, BSIZE + 1 = its size = its extent, ISIZE = its input bytes
__global__ __launch_bounds__(256) void bgzf_check_kernel(const uint64_t *nDev, uint64_t nHost, uint64_t capBytes,
                                                         const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ offs,
                                                         const uint8_t *__restrict__ packed, uint64_t packedCap, Result *res) {
    const uint64_t n = inputBytes(nDev, nHost, capBytes), nBlocks = (n + kBlockIn - 1) / kBlockIn;
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= nBlocks) return;
    const uint64_t s = offs[k], e = offs[k + 1];
    const uint32_t m = (uint32_t)(n - k * kBlockIn < kBlockIn ? n - k * kBlockIn : kBlockIn);
    bool ok = e >= s + 26 && e - s == sizes[k] && e - s <= m + 31 && e <= packedCap;
    if (ok) {
        const uint32_t bsize = (uint32_t)packed[s + 16] | (uint32_t)packed[s + 17] << 8;
        uint32_t isize = 0;
        for (uint32_t b = 0; b < 4; b++) isize |= (uint32_t)packed[e - 4 + b] << (8 * b);
        ok = packed[s] == 31 && packed[s + 1] == 139 && bsize + 1 == e - s && isize == m;
    }
    if (!ok) atomicAdd(&res->bad, 1u);
}

}  // namespace

hipError_t launch(const uint8_t *in, const uint64_t *nDev, uint64_t n, uint64_t capBytes, const Buffers &B,
                  hipStream_t st, hipEvent_t afterCompress, hipEvent_t afterScan) {
    hipError_t e = hipMemsetAsync(B.res, 0, sizeof(Result), st);
    if (e != hipSuccess) return e;
    const uint64_t maxBlocks = blocksOf(nDev ? capBytes : (n < capBytes ? n : capBytes));
    if (maxBlocks == 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_compress_kernel, dim3(B.grid), dim3(kThreads), 0, st, in, nDev, n, capBytes, B.slots, B.sizes,
                       B.tokens, B.res);
    if (afterCompress && (e = hipEventRecord(afterCompress, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(kThreads), 0, st, nDev, n, capBytes, B.sizes, B.offs, B.res);
    if (afterScan && (e = hipEventRecord(afterScan, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(bgzf_gather_kernel, dim3((unsigned)maxBlocks), dim3(256), 0, st, nDev, n, capBytes, B.slots, B.sizes,
                       B.offs, B.packed);
    hipLaunchKernelGGL(bgzf_check_kernel, dim3((unsigned)((maxBlocks + 255) / 256)), dim3(256), 0, st, nDev, n, capBytes,
                       B.sizes, B.offs, B.packed, maxBlocks * (uint64_t)kSlot, B.res);
    return hipGetLastError();
}

}  // namespace bgzfgpu
