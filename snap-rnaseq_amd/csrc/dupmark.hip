// dupmark.hip -- duplicate marking over a resident, coordinate-sorted BAM record stream, on the GPU with
// the rule of dupmark_rule.h (host model: host/dupmark.cpp).
//
//   fields + score  kLanes lanes per record: the fields, what the stream refuses, the sum of QUAL (dword
//                   loads over the aligned middle, bytes at the head and tail, a shuffle reduction);
//                   considered, strand, and a head flag where (refID, pos) differs from the record before
//   run numbering   a scan of the head flags: the records of one location carry one run index
//   best per group  64-bit atomicMax of rank(score, slot) and an atomicAdd of the size into
//                   [2 * run + strand], a workgroup's run-mates reduced in LDS first
//   mark            byte 19 of every accepted record: 0x400 set when it is considered and not its
//                   group's best, cleared otherwise; the marked count reduced per workgroup
//   check           the sum over groups of size - 1 and the groups of two or more
#include "dupmark.h"

#include <cstring>
#include <rocprim/rocprim.hpp>

using namespace baiindex;
using namespace duprule;

namespace dupgpu {

namespace {

constexpr uint32_t kConsidered = 1, kStrand = 2, kLocated = 4, kAccepted = 8;   // bits of info[i]
constexpr uint32_t kNoRun = 0xffffffffu;

struct Ptrs {
    uint32_t *score, *info, *head, *runIdx, *size;
    unsigned long long *best;
    Result *res;
};

Ptrs carve(char *w, const Layout &L) {
    Ptrs P;
    P.score = (uint32_t *)(w + L.score); P.info = (uint32_t *)(w + L.info);
    P.head = (uint32_t *)(w + L.head); P.runIdx = (uint32_t *)(w + L.runIdx);
    P.best = (unsigned long long *)(w + L.best); P.size = (uint32_t *)(w + L.size);
    P.res = (Result *)(w + L.res);
    return P;
}

// A record as the marking uses it.  A refused record has no location and no score.
struct Seen {
    uint64_t key, qualAt;   // sortKey; QUAL's offset in the record
    uint32_t flag, lSeq;
    bool refused, located, considered;
};

__device__ Seen see(const uint8_t *text, const uint64_t *start, uint64_t i, uint32_t nRef) {
    const uint64_t s = start[i], bytes = start[i + 1] - s;
    const uint8_t *rec = text + s;
    Seen v{~0ull, 0, 0, 0, true, false, false};
    if (bytes < kFixed || (uint64_t)load32(rec) + 4 != bytes) return v;
    const Fields f = fields(rec);
    if (!holdsCigar(f, bytes)) return v;
    if (refusal(f, (int64_t)f.pos + span(rec, f), nRef) != kOk) return v;
    const uint32_t lSeq = seqLen(rec);
    if (lSeq > kMaxSeq || !holdsQual(f, lSeq, bytes)) return v;
    v.key = sortKey(f.refID, f.pos);
    v.qualAt = qualOffset(f, lSeq);
    v.flag = f.flag;
    v.lSeq = lSeq;
    v.refused = false;
    v.located = f.refID >= 0;
    v.considered = considered(f);
    return v;
}

__global__ __launch_bounds__(kThreads) void dup_score_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start,
                                                             uint64_t n, uint32_t nRef, Ptrs P) {
    const uint32_t sub = threadIdx.x % kLanes;
    const uint64_t i = (uint64_t)blockIdx.x * kScoreRecords + threadIdx.x / kLanes;
    Seen v{~0ull, 0, 0, 0, true, false, false};
    uint32_t sum = 0;
    if (i < n) {
        v = see(text, start, i, nRef);
        if (v.considered) {
            const uint8_t *q = text + start[i] + v.qualAt;
            // [q, q + lSeq): up to 3 bytes to the first aligned dword, the dwords, up to 3 bytes behind them
            uint32_t headBytes = (4 - (uint32_t)((uintptr_t)q & 3)) & 3;
            if (headBytes > v.lSeq) headBytes = v.lSeq;
            const uint32_t nWords = (v.lSeq - headBytes) / 4, tailBytes = v.lSeq - headBytes - 4 * nWords;
            if (sub < headBytes) sum += qualValue(q[sub]);
            const uint32_t *w = (const uint32_t *)(q + headBytes);
            for (uint32_t k = sub; k < nWords; k += kLanes) sum += qualValue4(w[k]);
            const uint8_t *tail = q + headBytes + 4 * (uint64_t)nWords;
            if (sub < tailBytes) sum += qualValue(tail[sub]);
        }
    }
    // the kLanes lanes of a record run the same branches: all of them are here
    for (uint32_t m = kLanes / 2; m; m >>= 1) sum += __shfl_xor(sum, m, kLanes);
    if (sub) return;
    if (i < n) {
        Seen prev{~0ull, 0, 0, 0, false, false, false};
        if (i) prev = see(text, start, i - 1, nRef);
        if (v.refused || (i && !prev.refused && v.key < prev.key)) atomicAdd(&P.res->refused, 1u);
        if (!v.refused && (v.flag & kMateFlag)) atomicAdd(&P.res->mates, 1u);
        P.score[i] = sum;
        P.info[i] = (v.considered ? kConsidered : 0) | (strand(v.flag) ? kStrand : 0) | (v.located ? kLocated : 0) |
                    (v.refused ? 0 : kAccepted);
        P.head[i] = v.located && (i == 0 || !prev.located || prev.key != v.key);
    } else if (i == n) {
        P.head[n] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void dup_best_kernel(uint64_t n, Ptrs P) {
    __shared__ uint32_t sRun[kThreads];
    __shared__ uint64_t sRank[kThreads];   // 0: not considered
    __shared__ uint8_t sStrand[kThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t t = threadIdx.x;
    sRun[t] = kNoRun;
    sRank[t] = 0;
    sStrand[t] = 0;
    if (i < n) {
        const uint32_t info = P.info[i];
        if (info & kLocated) sRun[t] = P.runIdx[i] + P.head[i] - 1;   // the first located record is a head
        if (info & kConsidered) sRank[t] = rank(P.score[i], (uint32_t)i);
        sStrand[t] = (info & kStrand) ? 1 : 0;
    }
    __syncthreads();
    // one atomic pair per strand of a run in this workgroup, not one per record
    if (sRun[t] != kNoRun && (t == 0 || sRun[t - 1] != sRun[t])) {
        const uint32_t r = sRun[t];
        uint64_t best[2] = {0, 0};
        uint32_t size[2] = {0, 0};
        for (uint32_t k = t; k < kThreads && sRun[k] == r; k++) {
            if (!sRank[k]) continue;
            const uint32_t s = sStrand[k];
            if (sRank[k] > best[s]) best[s] = sRank[k];
            size[s]++;
        }
        for (uint32_t s = 0; s < 2; s++)
            if (size[s]) {
                atomicMax(&P.best[2 * (uint64_t)r + s], (unsigned long long)best[s]);
                atomicAdd(&P.size[2 * (uint64_t)r + s], size[s]);
            }
    }
}

__global__ __launch_bounds__(kThreads) void dup_mark_kernel(uint8_t *__restrict__ text, const uint64_t *__restrict__ start,
                                                            uint64_t n, Ptrs P) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool marked = false;
    const uint32_t info = i < n ? P.info[i] : 0;
    if (info & kAccepted) {
        if (info & kConsidered) {
            const uint64_t g = 2 * (uint64_t)(P.runIdx[i] + P.head[i] - 1) + ((info & kStrand) ? 1 : 0);
            marked = rank(P.score[i], (uint32_t)i) != P.best[g];
        }
        uint8_t *b = text + start[i] + kFlagHighByte;
        *b = flagByte(*b, marked);
    }
    const int count = __syncthreads_count(marked);
    if (threadIdx.x == 0 && count) atomicAdd(&P.res->marked, (unsigned long long)count);
}

// Over the 2 * runs (run, strand) groups.
__global__ __launch_bounds__(kThreads) void dup_check_kernel(uint64_t n, Ptrs P) {
    __shared__ uint32_t sDup[kThreads];
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t t = threadIdx.x;
    const uint32_t size = g < 2 * (uint64_t)P.runIdx[n] ? P.size[g] : 0;
    sDup[t] = size ? size - 1 : 0;
    const int groups = __syncthreads_count(size >= 2);
    for (uint32_t d = kThreads / 2; d; d >>= 1) {
        if (t < d) sDup[t] += sDup[t + d];
        __syncthreads();
    }
    if (t == 0 && sDup[0]) atomicAdd(&P.res->expected, (unsigned long long)sDup[0]);
    if (t == 0 && groups) atomicAdd(&P.res->groups, (unsigned long long)groups);
}

inline unsigned blocksFor(uint64_t items, uint32_t per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

hipError_t tempBytes(uint64_t n, hipStream_t st, uint64_t *bytes) {
    size_t scan = 0;
    *bytes = 0;
    if (n == 0) return hipSuccess;
    const hipError_t e = rocprim::exclusive_scan(nullptr, scan, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n + 1,
                                                 rocprim::plus<uint32_t>(), st);
    *bytes = scan;
    return e;
}

Layout layout(uint64_t n, uint64_t temp) {
    Layout L{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at = (at + bytes + 15) & ~15ull;
        return here;
    };
    L.score = take(n * 4); L.info = take(n * 4);
    L.head = take((n + 1) * 4); L.runIdx = take((n + 1) * 4);
    L.best = take(2 * n * 8); L.size = take(2 * n * 4);
    L.tempBytes = temp;
    L.temp = take(temp);
    L.res = take(sizeof(Result));
    L.bytes = at;
    return L;
}

hipError_t launch(uint8_t *text, const uint64_t *start, uint64_t n, uint32_t nRef, char *work, const Layout &L, hipStream_t st,
                  hipEvent_t *ev) {
    const Ptrs P = carve(work, L);
    auto mark = [&](int k) { return ev ? hipEventRecord(ev[k], st) : hipSuccess; };
    hipError_t e;
#define DUP_TRY(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
    DUP_TRY(mark(0));
    DUP_TRY(hipMemsetAsync(P.res, 0, sizeof(Result), st));
    if (n) {
        hipLaunchKernelGGL(dup_score_kernel, dim3(blocksFor(n + 1, kScoreRecords)), dim3(kThreads), 0, st, text, start, n, nRef, P);
        DUP_TRY(mark(1));
        size_t temp = L.tempBytes;
        DUP_TRY(rocprim::exclusive_scan(work + L.temp, temp, P.head, P.runIdx, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
        DUP_TRY(mark(2));
        DUP_TRY(hipMemsetAsync(P.best, 0, 2 * n * 8, st));
        DUP_TRY(hipMemsetAsync(P.size, 0, 2 * n * 4, st));
        hipLaunchKernelGGL(dup_best_kernel, dim3(blocksFor(n, kThreads)), dim3(kThreads), 0, st, n, P);
        DUP_TRY(mark(3));
        hipLaunchKernelGGL(dup_mark_kernel, dim3(blocksFor(n, kThreads)), dim3(kThreads), 0, st, text, start, n, P);
        DUP_TRY(mark(4));
        hipLaunchKernelGGL(dup_check_kernel, dim3(blocksFor(2 * n, kThreads)), dim3(kThreads), 0, st, n, P);
    } else {
        for (int k = 1; k < kPasses; k++) DUP_TRY(mark(k));
    }
    DUP_TRY(mark(kPasses));
#undef DUP_TRY
    return hipGetLastError();
}

}  // namespace dupgpu
