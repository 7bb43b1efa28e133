// index_build.hip -- the seed index built on the device (snapgpu_index_build_gpu), byte-identical
// to the CPU builder of host/index.cpp (snapgpu_index_build_ex), which defines "correct".
//
//   scan       one record per genome position: (canonical seed << 1 | side, position); positions
//              without a valid seed get a key of all ones, which sorts last
//   sort       stable radix sort by key (rocPRIM): (canonical seed, side, position) order, i.e. the
//              CPU's per-table (key, position) order with tables concatenated and each key's
//              side-0 positions before its side-1 positions
//   runs       segment = equal (seed, side), run = equal seed (1 or 2 segments).  Two scans give
//              every segment's start, every run's first segment and every segment's overflow
//              offset; a segment of n > 1 positions takes 1 + n overflow words, in exactly the
//              order the CPU emits them (tables ascending, keys ascending, side 0 then 1)
//   sizing     per-table distinct keys and overflow words go to the host, which runs the same
//              double arithmetic as the CPU builder (sizeTables, host/index.cpp)
//   placement  priority claiming over per-slot owner words (index_place.h)
//   write      slots from the owner words, overflow runs [count, positions descending]
// All element indices are 64-bit: a human-sized genome has more than 2^31 positions.
#include <cstring>
#include <cstdlib>
#include <rocprim/rocprim.hpp>

#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "index_place.h"
#include "internal.h"
#include "large_copy.h"

namespace {

using snapgpu::kPlaceNone;

constexpr int kBlock = 256;
constexpr int kItems = 8;                          // per thread in the scans
constexpr uint64_t kTile = (uint64_t)kBlock * kItems;
constexpr uint64_t kNoSeed = ~0ull;                // key of a position without a valid seed

struct Counters {
    unsigned long long valid;                      // positions with a seed
    uint32_t iupac;                                // a byte outside ACGTn
    uint32_t placeErrors;                          // probe walks that overran their bound
};

// Tables.cpp:41-48 (baseValue of host/internal.h)
__device__ __forceinline__ uint32_t baseValueDev(char c) {
    return c == 'A' ? 0u : c == 'G' ? 1u : c == 'C' ? 2u : c == 'T' ? 3u : 4u;
}

// A block owns 256 consecutive positions (a wave: one 64-aligned stretch of 64).  It stages the
// 2-bit values of its 256 + L - 1 bases in LDS; each thread then rolls its own seed and reverse
// complement out of them (Seed.h:38-51: first base in the highest bits), exactly forEachSeed's
// fw and rc once its run has reached L.  A seed depends on its own L bases only, so a stretch
// needs no state from the one before it.  Loads and stores are coalesced.
__global__ __launch_bounds__(kBlock) void seedScanKernel(const char *__restrict__ g, uint32_t nBases, uint64_t nPos,
                                                         uint32_t L, uint64_t *__restrict__ K, uint32_t *__restrict__ P,
                                                         Counters *c) {
    __shared__ uint8_t v[kBlock + 32];
    const uint64_t base = (uint64_t)blockIdx.x * kBlock;
    int iupac = 0;
    for (uint32_t j = threadIdx.x; j < kBlock + L - 1; j += kBlock) {
        const uint64_t p = base + j;
        const char ch = p < nBases ? g[p] : 'n';
        v[j] = (uint8_t)baseValueDev(ch);
        if (j < kBlock && ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'n') iupac = 1;
    }
    __syncthreads();
    const uint64_t p = base + threadIdx.x;
    int valid = 0;
    if (p < nPos) {
        uint64_t fw = 0, rc = 0;
        uint32_t bad = 0;
        for (uint32_t i = 0; i < L; i++) {
            const uint32_t b = v[threadIdx.x + i];
            bad |= b >> 2;
            fw = (fw << 2) | (b & 3);
            rc = (rc >> 2) | ((uint64_t)((b & 3) ^ 3) << (2 * (L - 1)));
        }
        valid = !bad;
        K[p] = bad ? kNoSeed : (((fw > rc ? rc : fw) << 1) | (uint64_t)(fw > rc));
        P[p] = (uint32_t)p;
    }
    const int nValid = __syncthreads_count(valid);
    const int anyIupac = __syncthreads_or(iupac);
    if (threadIdx.x == 0) {
        if (nValid) atomicAdd(&c->valid, (unsigned long long)nValid);
        if (anyIupac) atomicOr(&c->iupac, 1u);
    }
}

// ---------------------------------------------------------------- scans over 64-bit sums
// Exclusive prefix of x over the block's 256 threads; *total = the block's sum.
__device__ __forceinline__ uint64_t blockExclusiveScan(uint64_t x, uint64_t *total) {
    __shared__ uint64_t sh[kBlock];
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const uint64_t y = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[kBlock - 1];
    __syncthreads();
    return incl - x;
}

// tileSum[tile] = sum of f(i) over the tile's kTile elements
template <class F>
__global__ __launch_bounds__(kBlock) void tileReduceKernel(F f, uint64_t n, uint64_t *tileSum) {
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    uint64_t s = 0;
    for (int k = 0; k < kItems; k++)
        if (i0 + k < n) s += f(i0 + k);
    uint64_t total;
    blockExclusiveScan(s, &total);
    if (threadIdx.x == 0) tileSum[blockIdx.x] = total;
}

// One block: tileSum[0 .. nTiles) -> its exclusive prefix in place, tileSum[nTiles] = the total.
__global__ __launch_bounds__(kBlock) void scanTileSumsKernel(uint64_t *tileSum, uint64_t nTiles) {
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nTiles; base += kTile) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kItems;
        uint64_t x[kItems], s = 0;
        for (int k = 0; k < kItems; k++) { x[k] = i0 + k < nTiles ? tileSum[i0 + k] : 0; s += x[k]; }
        uint64_t total;
        uint64_t run = carry + blockExclusiveScan(s, &total);
        for (int k = 0; k < kItems; k++)
            if (i0 + k < nTiles) { tileSum[i0 + k] = run; run += x[k]; }
        carry += total;
    }
    if (threadIdx.x == 0) tileSum[nTiles] = carry;
}

// out(i, f(i), exclusive prefix of f at i), given the scanned tile sums
template <class F, class O>
__global__ __launch_bounds__(kBlock) void tileScanKernel(F f, O out, uint64_t n, const uint64_t *tileSum) {
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    uint64_t x[kItems], s = 0;
    for (int k = 0; k < kItems; k++) { x[k] = i0 + k < n ? f(i0 + k) : 0; s += x[k]; }
    uint64_t total;
    uint64_t run = tileSum[blockIdx.x] + blockExclusiveScan(s, &total);
    for (int k = 0; k < kItems; k++)
        if (i0 + k < n) { out(i0 + k, x[k], run); run += x[k]; }
}

// Head flags of sorted record i: bit 0 a new segment (seed, side), bit 32 a new run (seed).  Both
// counts stay below 2^32 (at most one per genome position), so one 64-bit sum carries the two.
struct HeadFlags {
    const uint64_t *K;
    __device__ uint64_t operator()(uint64_t i) const {
        if (i == 0) return 1ull | (1ull << 32);
        const uint64_t a = K[i - 1], b = K[i];
        return (uint64_t)(a != b) | ((uint64_t)((a >> 1) != (b >> 1)) << 32);
    }
};
struct HeadOut {
    uint32_t *segIdx, *segStart, *runFirstSeg;
    __device__ void operator()(uint64_t i, uint64_t flags, uint64_t excl) const {
        const uint64_t incl = excl + flags;
        const uint32_t s = (uint32_t)incl - 1;
        segIdx[i] = s;
        if (flags & 1) segStart[s] = (uint32_t)i;
        if (flags >> 32) runFirstSeg[(uint32_t)(incl >> 32) - 1] = s;
    }
};
// Overflow words of segment s: [count, positions] when it has more than one position
struct OvfWords {
    const uint32_t *segStart;
    __device__ uint64_t operator()(uint64_t s) const {
        const uint64_t n = segStart[s + 1] - segStart[s];
        return n > 1 ? 1 + n : 0;
    }
};
struct OvfOut {
    uint64_t *ovfOff;
    __device__ void operator()(uint64_t s, uint64_t, uint64_t excl) const { ovfOff[s] = excl; }
};

// What the run kernels read: sorted records, segments, runs.  segStart[nSeg] = nValid,
// runFirstSeg[nRun] = nSeg, ovfOff[nSeg] = all overflow words.
struct Runs {
    const uint64_t *K;
    const uint32_t *P;
    const uint32_t *segIdx, *segStart, *runFirstSeg;
    const uint64_t *ovfOff;
    uint64_t nValid, nSeg, nRun;
    __device__ uint64_t canon(uint64_t r) const { return K[segStart[runFirstSeg[r]]] >> 1; }
};

// distinct keys and overflow words of table tb = canonical seed >> 32: runs are in table order, so
// a table's runs are [lowerBound(tb), lowerBound(tb + 1))
__global__ __launch_bounds__(kBlock) void tableStatsKernel(Runs R, uint32_t nTables, uint64_t *distinct, uint64_t *ovfWords) {
    const uint64_t tb = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tb >= nTables) return;
    uint64_t bound[2];
    for (int k = 0; k < 2; k++) {
        uint64_t lo = 0, hi = R.nRun;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((R.canon(mid) >> 32) < tb + k) lo = mid + 1; else hi = mid;
        }
        bound[k] = lo;
    }
    distinct[tb] = bound[1] - bound[0];
    ovfWords[tb] = R.ovfOff[R.runFirstSeg[bound[1]]] - R.ovfOff[R.runFirstSeg[bound[0]]];
}

__global__ __launch_bounds__(kBlock) void fillKernel(uint32_t *p, uint64_t n, uint32_t value) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = value;
}

// One thread per run: claim a slot for its key (index_place.h).  The rank is the global run
// index: within a table that is ascending key order, and tables do not share slots.
__global__ __launch_bounds__(kBlock) void placeKernel(Runs R, const uint64_t *tableBase, const uint64_t *tableSize,
                                                      uint32_t *owner, Counters *c) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= R.nRun) return;
    const uint64_t tb = R.canon(g) >> 32;
    uint32_t *own = owner + tableBase[tb];
    const bool ok = snapgpu::placeClaim(
        (uint32_t)g, tableSize[tb], [&](uint64_t i, uint32_t r) { return atomicMin(&own[i], r); },
        [&](uint32_t r) { return (uint32_t)R.canon(r); });
    if (!ok) atomicAdd(&c->placeErrors, 1u);
}

// One thread per slot: the empty pattern (HashTable.cpp:72-75) or (key, value1, value2) of the
// run that owns it.  A side's value: kUnusedSide without a position, the position when it has
// one, nBases + its overflow offset when it has more (GenomeIndex.cpp:546-619).
__global__ __launch_bounds__(kBlock) void writeSlotsKernel(Runs R, const uint32_t *owner, uint64_t nSlots, uint32_t nBases,
                                                           uint32_t *slots) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nSlots) return;
    const uint32_t g = owner[i];
    uint32_t key = 0, v0 = snapgpu::kInvalidLocation, v1 = 0;
    if (g != kPlaceNone) {
        const uint32_t s0 = R.runFirstSeg[g], s1 = R.runFirstSeg[g + 1];
        v0 = v1 = snapgpu::kUnusedSide;
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t a = R.segStart[s], n = R.segStart[s + 1] - a;
            const uint64_t k = R.K[a];
            key = (uint32_t)(k >> 1);
            const uint32_t v = n == 1 ? R.P[a] : nBases + (uint32_t)R.ovfOff[s];
            if (k & 1) v1 = v; else v0 = v;
        }
    }
    slots[3 * i] = key;
    slots[3 * i + 1] = v0;
    slots[3 * i + 2] = v1;
}

// One thread per sorted record: its place in its segment's overflow run [count, positions
// descending] (positions ascend within a segment: the sort is stable)
__global__ __launch_bounds__(kBlock) void writeOverflowKernel(Runs R, uint32_t *ovf) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= R.nValid) return;
    const uint32_t s = R.segIdx[i];
    const uint64_t a = R.segStart[s], n = R.segStart[s + 1] - a;
    if (n <= 1) return;
    const uint64_t off = R.ovfOff[s], j = i - a;
    if (j == 0) ovf[off] = (uint32_t)n;
    ovf[off + 1 + (n - 1 - j)] = R.P[i];
}

uint32_t blocksFor(uint64_t n, uint64_t per) { return (uint32_t)((n + per - 1) / per); }

// Device allocations of one build: freed on every path, the most held at once recorded.
struct DeviceArena {
    std::vector<std::pair<void *, uint64_t>> live;
    uint64_t held = 0, peak = 0;
    ~DeviceArena() { for (auto &a : live) hipFree(a.first); }
    void release(void *p) {
        for (auto &a : live)
            if (a.first == p && p) { hipFree(p); held -= a.second; a.first = nullptr; a.second = 0; }
    }
};

std::mutex g_statsMu;                              // builds may run on several threads
double g_phase[SNAPGPU_INDEX_BUILD_PHASES];
uint64_t g_peak = 0;
bool g_haveStats = false;

}  // namespace

extern "C" int snapgpu_index_build_gpu_stats(double phaseSeconds[SNAPGPU_INDEX_BUILD_PHASES], uint64_t *peakDeviceBytes) {
    std::lock_guard<std::mutex> lock(g_statsMu);
    if (!g_haveStats) { snapgpu::setError("index_build_gpu_stats: no GPU index build in this process"); return SNAPGPU_EINVAL; }
    if (phaseSeconds) memcpy(phaseSeconds, g_phase, sizeof(g_phase));
    if (peakDeviceBytes) *peakDeviceBytes = g_peak;
    return SNAPGPU_OK;
}

extern "C" snapgpu_index_t *snapgpu_index_build_gpu(snapgpu_genome_t *genome, int seedLen, double slack, int device) {
    using snapgpu::setError;
    if (!genome || seedLen < 16 || seedLen > 31) { setError("index_build_gpu: seedLen must be 16..31"); delete genome; return nullptr; }
    if (!(slack > 0)) slack = 0.3;   // GenomeIndex.cpp:208 default
    int nDev = 0, prevDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess) nDev = 0;
    if (device < 0 || device >= nDev) {
        setError("index_build_gpu: no HIP device " + std::to_string(device) + " (" + std::to_string(nDev) + " visible)");
        delete genome;
        return nullptr;
    }
    auto *idx = new snapgpu_index_t();
    idx->genome = genome;
    idx->seedLen = (uint32_t)seedLen;
    idx->nTables = 1u << ((seedLen - 16) * 2);
    const uint32_t L = (uint32_t)seedLen, nT = idx->nTables, nBases = genome->nBases;
    if (nBases > 0xfffffff0u) { setError("genome too big"); delete idx; return nullptr; }
    const uint64_t nPos = nBases > L + 1 ? (uint64_t)nBases - L - 1 : 0;   // as snapgpu_index_build_ex

    hipGetDevice(&prevDev);
    DeviceArena arena;
    hipStream_t stream = nullptr;
    bool failed = false;
    auto fail = [&](const std::string &msg) { if (!failed) setError("index_build_gpu: " + msg); failed = true; return false; };
    auto hip = [&](hipError_t e, const char *what) {
        if (e == hipSuccess) return true;
        return fail(std::string(what) + ": " + hipGetErrorString(e));
    };
    // hipMemGetInfo before a group of allocations: the group must fit in what is free now
    auto reserve = [&](uint64_t bytes, const char *what) {
        size_t freeB = 0, totalB = 0;
        if (!hip(hipMemGetInfo(&freeB, &totalB), "hipMemGetInfo")) return false;
        if (bytes > freeB)
            return fail(std::string("out of device memory (SNAPGPU_ENOMEM) for ") + what + ": " + std::to_string(bytes) +
                        " bytes needed, " + std::to_string(freeB) + " bytes free");
        return true;
    };
    auto alloc = [&](auto **p, uint64_t bytes, const char *what) {
        void *q = nullptr;
        const uint64_t b = bytes ? bytes : 16;
        const hipError_t e = hipMalloc(&q, b);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            size_t freeB = 0, totalB = 0;
            hipGetLastError();
            hipMemGetInfo(&freeB, &totalB);
            return fail(std::string("out of device memory (SNAPGPU_ENOMEM) for ") + what + ": " + std::to_string(b) +
                        " bytes needed, " + std::to_string(freeB) + " bytes free");
        }
        if (!hip(e, what)) return false;
        arena.live.emplace_back(q, b);
        arena.held += b;
        if (arena.held > arena.peak) arena.peak = arena.held;
        *p = static_cast<std::remove_reference_t<decltype(*p)>>(q);
        return true;
    };
    double phase[SNAPGPU_INDEX_BUILD_PHASES] = {0};
    auto tPrev = std::chrono::steady_clock::now();
    // end of a phase: the stream drained, the kernels' errors seen, the wall time booked
    auto endPhase = [&](int k, const char *what) {
        if (!hip(hipGetLastError(), what) || !hip(hipStreamSynchronize(stream), what)) return false;
        const auto t = std::chrono::steady_clock::now();
        phase[k] += std::chrono::duration<double>(t - tPrev).count();
        tPrev = t;
        return true;
    };

    char *dG = nullptr;
    uint64_t *K0 = nullptr, *K1 = nullptr, *tileSum = nullptr, *dDistinct = nullptr, *dOvfWords = nullptr;
    uint64_t *dTableBase = nullptr, *dTableSize = nullptr;
    uint32_t *P0 = nullptr, *P1 = nullptr, *segStart = nullptr, *runFirstSeg = nullptr, *owner = nullptr;
    uint32_t *dSlots = nullptr, *dOvf = nullptr;
    void *sortTemp = nullptr;
    Counters *dC = nullptr;
    Counters hC{};
    // host ends of small asynchronous copies: they outlive every path to the clean-up's synchronise
    uint64_t heads = 0, totalOverflow = 0;
    uint32_t endSeg = 0, endRun = 0;

    // do { ... } while (0): every failure breaks out to the one clean-up below
    do {
        if (!hip(hipSetDevice(device), "hipSetDevice") || !hip(hipStreamCreate(&stream), "hipStreamCreate")) break;
        // ---- phase 0: upload
        size_t sortBytes = 0;
        const unsigned endBit = 2 * L + 1;
        {
            rocprim::double_buffer<uint64_t> qk(K0, K1);
            rocprim::double_buffer<uint32_t> qv(P0, P1);
            if (nPos && !hip(rocprim::radix_sort_pairs(nullptr, sortBytes, qk, qv, (size_t)nPos, 0u, endBit, stream),
                             "radix_sort_pairs (size query)")) break;
        }
        const uint64_t nRec = nPos + 2;   // room for the sentinels segStart[nSeg], ovfOff[nSeg] kept in these buffers
        const uint64_t nTiles = (nPos + kTile - 1) / kTile;
        if (!reserve((uint64_t)nBases + 2 * nRec * 12 + sortBytes + (nTiles + 1) * 8 + sizeof(Counters) + 4096, "the seed records")) break;
        if (!alloc(&dG, nBases, "genome") || !alloc(&K0, nRec * 8, "keys") || !alloc(&P0, nRec * 4, "positions") ||
            !alloc(&K1, nRec * 8, "keys (second buffer)") || !alloc(&P1, nRec * 4, "positions (second buffer)") ||
            !alloc(&sortTemp, sortBytes, "sort storage") || !alloc(&tileSum, (nTiles + 1) * 8, "tile sums") ||
            !alloc(&dC, sizeof(Counters), "counters")) break;
        if (!hip(hipMemsetAsync(dC, 0, sizeof(Counters), stream), "hipMemsetAsync")) break;
        if (snapgpu::uploadLarge(stream, dG, genome->bases(), nBases) != SNAPGPU_OK) { failed = true; break; }
        if (!endPhase(0, "upload")) break;
        // ---- phase 1: scan
        if (nBases) seedScanKernel<<<blocksFor(nBases, kBlock), kBlock, 0, stream>>>(dG, nBases, nPos, L, K0, P0, dC);
        if (!hip(hipGetLastError(), "seedScanKernel")) break;
        if (!hip(hipMemcpyAsync(&hC, dC, sizeof(Counters), hipMemcpyDeviceToHost, stream), "counters")) break;
        if (!endPhase(1, "scan")) break;
        const uint64_t nValid = hC.valid;
        idx->hasIupac = hC.iupac != 0;
        // ---- phase 2: sort
        // the two record buffers are the sort's ping and pong: no third copy in its storage
        rocprim::double_buffer<uint64_t> dk(K0, K1);
        rocprim::double_buffer<uint32_t> dv(P0, P1);
        if (nPos && !hip(rocprim::radix_sort_pairs(sortTemp, sortBytes, dk, dv, (size_t)nPos, 0u, endBit, stream),
                         "radix_sort_pairs")) break;
        if (!endPhase(2, "sort")) break;
        arena.release(sortTemp);
        arena.release(dG);
        const uint64_t *Ks = dk.current();
        const uint32_t *Ps = dv.current();
        // ---- phase 3: runs.  The buffers the sort left over hold segIdx and ovfOff.
        uint32_t *segIdx = dv.alternate();
        uint64_t *ovfOff = dk.alternate();
        uint64_t nSeg = 0, nRun = 0;
        const uint32_t vTiles = blocksFor(nValid, kTile);
        if (nValid) {
            tileReduceKernel<<<vTiles, kBlock, 0, stream>>>(HeadFlags{Ks}, nValid, tileSum);
            scanTileSumsKernel<<<1, kBlock, 0, stream>>>(tileSum, vTiles);
            if (!hip(hipGetLastError(), "head flag sums") ||
                !hip(hipMemcpyAsync(&heads, tileSum + vTiles, 8, hipMemcpyDeviceToHost, stream), "head flag total") ||
                !hip(hipStreamSynchronize(stream), "head flag total")) break;
            nSeg = heads & 0xffffffffull;
            nRun = heads >> 32;
        }
        if (!reserve((nSeg + nRun + 2) * 4 + 4ull * nT * 8 + 4096, "the run tables")) break;
        if (!alloc(&segStart, (nSeg + 1) * 4, "segment starts") || !alloc(&runFirstSeg, (nRun + 1) * 4, "run starts") ||
            !alloc(&dDistinct, (uint64_t)nT * 8, "distinct") || !alloc(&dOvfWords, (uint64_t)nT * 8, "overflow words") ||
            !alloc(&dTableBase, (uint64_t)nT * 8, "table bases") || !alloc(&dTableSize, (uint64_t)nT * 8, "table sizes")) break;
        endSeg = (uint32_t)nValid;
        endRun = (uint32_t)nSeg;
        if (!hip(hipMemcpyAsync(segStart + nSeg, &endSeg, 4, hipMemcpyHostToDevice, stream), "segStart end") ||
            !hip(hipMemcpyAsync(runFirstSeg + nRun, &endRun, 4, hipMemcpyHostToDevice, stream), "runFirstSeg end")) break;
        if (nValid) {
            tileScanKernel<<<vTiles, kBlock, 0, stream>>>(HeadFlags{Ks}, HeadOut{segIdx, segStart, runFirstSeg}, nValid, tileSum);
            const uint32_t sTiles = blocksFor(nSeg, kTile);
            tileReduceKernel<<<sTiles, kBlock, 0, stream>>>(OvfWords{segStart}, nSeg, tileSum);
            scanTileSumsKernel<<<1, kBlock, 0, stream>>>(tileSum, sTiles);
            tileScanKernel<<<sTiles, kBlock, 0, stream>>>(OvfWords{segStart}, OvfOut{ovfOff}, nSeg, tileSum);
            if (!hip(hipGetLastError(), "overflow offsets") ||
                !hip(hipMemcpyAsync(&totalOverflow, tileSum + sTiles, 8, hipMemcpyDeviceToHost, stream), "overflow total") ||
                !hip(hipStreamSynchronize(stream), "overflow total")) break;
        }
        if (!hip(hipMemcpyAsync(ovfOff + nSeg, &totalOverflow, 8, hipMemcpyHostToDevice, stream), "ovfOff end")) break;
        const Runs R{Ks, Ps, segIdx, segStart, runFirstSeg, ovfOff, nValid, nSeg, nRun};
        tableStatsKernel<<<blocksFor(nT, kBlock), kBlock, 0, stream>>>(R, nT, dDistinct, dOvfWords);
        if (!endPhase(3, "runs")) break;
        // ---- phase 4: sizing, on the host
        std::vector<uint64_t> distinct(nT), ovfWords(nT), ovfBase;
        if (snapgpu::downloadLarge(stream, distinct.data(), dDistinct, (uint64_t)nT * 8) != SNAPGPU_OK ||
            snapgpu::downloadLarge(stream, ovfWords.data(), dOvfWords, (uint64_t)nT * 8) != SNAPGPU_OK) { failed = true; break; }
        const uint64_t totalSlots = snapgpu::sizeTables(*idx, slack, nValid, distinct.data(), ovfWords.data(), ovfBase);
        if (ovfBase[nT] != totalOverflow) { fail("per-table overflow words do not add up to the overflow scan"); break; }
        if ((uint64_t)nBases + totalOverflow > 0xfffffff0ull) { fail("overflow table namespace exhausted"); break; }
        if (snapgpu::uploadLarge(stream, dTableBase, idx->tableBase.data(), (uint64_t)nT * 8) != SNAPGPU_OK ||
            snapgpu::uploadLarge(stream, dTableSize, idx->tableSize.data(), (uint64_t)nT * 8) != SNAPGPU_OK) { failed = true; break; }
        if (!endPhase(4, "sizing")) break;
        // ---- phase 5: placement
        if (!reserve(totalSlots * 16 + totalOverflow * 4 + 4096, "the table image")) break;
        if (!alloc(&owner, totalSlots * 4, "slot owners") || !alloc(&dSlots, totalSlots * 12, "slots") ||
            !alloc(&dOvf, totalOverflow * 4, "overflow")) break;
        fillKernel<<<blocksFor(totalSlots, kBlock), kBlock, 0, stream>>>(owner, totalSlots, kPlaceNone);
        if (nRun) placeKernel<<<blocksFor(nRun, kBlock), kBlock, 0, stream>>>(R, dTableBase, dTableSize, owner, dC);
        if (!hip(hipGetLastError(), "placeKernel") ||
            !hip(hipMemcpyAsync(&hC, dC, sizeof(Counters), hipMemcpyDeviceToHost, stream), "counters")) break;
        if (!endPhase(5, "placement")) break;
        if (hC.placeErrors) { fail(std::to_string(hC.placeErrors) + " probe walks overran their bound (SNAPGPU_EDEVICE)"); break; }
        // ---- phase 6: write
        writeSlotsKernel<<<blocksFor(totalSlots, kBlock), kBlock, 0, stream>>>(R, owner, totalSlots, nBases, dSlots);
        if (nValid) writeOverflowKernel<<<blocksFor(nValid, kBlock), kBlock, 0, stream>>>(R, dOvf);
        if (!endPhase(6, "write")) break;
        // ---- phase 7: download
        idx->slots.allocate(3 * totalSlots);
        idx->overflow.allocate(totalOverflow);
        if (snapgpu::downloadLarge(stream, idx->slots.mut(), dSlots, totalSlots * 12) != SNAPGPU_OK ||
            snapgpu::downloadLarge(stream, idx->overflow.mut(), dOvf, totalOverflow * 4) != SNAPGPU_OK) { failed = true; break; }
        if (!endPhase(7, "download")) break;
    } while (0);

    if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
    for (auto &a : arena.live) if (a.first) { hipFree(a.first); a.first = nullptr; }
    hipSetDevice(prevDev);
    if (failed) { delete idx; return nullptr; }
    std::lock_guard<std::mutex> lock(g_statsMu);
    memcpy(g_phase, phase, sizeof(phase));
    g_peak = arena.peak;
    g_haveStats = true;
    return idx;
}
