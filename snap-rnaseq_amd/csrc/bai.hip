// bai.hip -- the BAI index of a resident, coordinate-sorted BAM record stream and its device BGZF
// members, built on the GPU with the rules of bai_index.h (host model: host/bai.cpp).
//
//   field pass     per record: refID, bin, span, start and end virtual offset; chunk heads and tails;
//                  reference boundaries; refused / unsorted records counted (always 0); mapped,
//                  unmapped and the largest end per reference, reduced per workgroup run first
//   chunk heads    a scan of the head flags compacts the chunks
//   sort           stable radix sort of the chunks on (refID << 16) | bin
//   counts         bin heads, their scan, per-reference chunk and bin ranges from segment boundaries
//   linear index   per-reference sizes and scans; each record's start into the windows it is the
//                  first to overlap (64-bit atomicMin); reverse first-defined-value scan
//   write          one kernel places every field of the file
//   check          the total recomputed from the counts
#include "bai.h"

#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>

using namespace baiindex;

namespace baigpu {

namespace {

__host__ __device__ inline uint64_t least(uint64_t a, uint64_t b) { return a < b ? a : b; }

struct Ptrs {
    int32_t *ref, *beg, *end;
    uint32_t *bin, *head, *tail, *headIdx;
    uint64_t *vbeg, *vend;
    uint64_t *key, *keySorted, *cbeg, *cend;
    uint32_t *val, *valSorted, *binHead, *binIdx, *binStart;
    RefInfo *info;
    uint64_t *refOff, *linBase, *lin;
    Result *res;
    uint64_t linCap;
};

Ptrs carve(char *w, const Layout &L) {
    Ptrs P;
    P.ref = (int32_t *)(w + L.ref); P.bin = (uint32_t *)(w + L.bin);
    P.beg = (int32_t *)(w + L.beg); P.end = (int32_t *)(w + L.end);
    P.vbeg = (uint64_t *)(w + L.vbeg); P.vend = (uint64_t *)(w + L.vend);
    P.head = (uint32_t *)(w + L.head); P.tail = (uint32_t *)(w + L.tail); P.headIdx = (uint32_t *)(w + L.headIdx);
    P.key = (uint64_t *)(w + L.key); P.keySorted = (uint64_t *)(w + L.keySorted);
    P.val = (uint32_t *)(w + L.val); P.valSorted = (uint32_t *)(w + L.valSorted);
    P.cbeg = (uint64_t *)(w + L.cbeg); P.cend = (uint64_t *)(w + L.cend);
    P.binHead = (uint32_t *)(w + L.binHead); P.binIdx = (uint32_t *)(w + L.binIdx); P.binStart = (uint32_t *)(w + L.binStart);
    P.info = (RefInfo *)(w + L.info); P.refOff = (uint64_t *)(w + L.refOff); P.linBase = (uint64_t *)(w + L.linBase);
    P.lin = (uint64_t *)(w + L.lin);
    P.res = (Result *)(w + L.res);
    P.linCap = L.linCap;
    return P;
}

// A record's fields as the index uses them: refused records count as records without a reference.
struct Seen {
    int32_t ref, pos;
    uint32_t bin, flag;
    int64_t end;
    bool refused;
};

__device__ Seen see(const uint8_t *text, const uint64_t *start, uint64_t i, uint32_t nRef) {
    const uint64_t s = start[i], bytes = start[i + 1] - s;
    const uint8_t *rec = text + s;
    Seen v{-1, 0, 0, 0, 1, true};
    if (bytes < kFixed || (uint64_t)load32(rec) + 4 != bytes) return v;
    const Fields f = fields(rec);
    if (!holdsCigar(f, bytes)) return v;
    v.end = (int64_t)f.pos + span(rec, f);
    if (refusal(f, v.end, nRef) != kOk) return v;
    v.ref = f.refID; v.pos = f.pos; v.bin = f.bin; v.flag = f.flag;
    v.refused = false;
    return v;
}

__global__ __launch_bounds__(kThreads) void bai_field_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start,
                                                             uint64_t n, uint32_t nRef, const uint64_t *__restrict__ coff,
                                                             uint64_t streamOffset, Ptrs P) {
    __shared__ int32_t sRef[kThreads], sEnd[kThreads];
    __shared__ uint32_t sUnmapped[kThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t t = threadIdx.x;
    sRef[t] = -1;
    if (i < n) {
        const Seen v = see(text, start, i, nRef);
        Seen prev{-1, 0, 0, 0, 1, false}, next{-1, 0, 0, 0, 1, false};
        if (i) prev = see(text, start, i - 1, nRef);
        if (i + 1 < n) next = see(text, start, i + 1, nRef);
        uint32_t bad = v.refused ? 1u : 0u;
        if (i && !v.refused && !prev.refused && sortKey(v.ref, v.pos) < sortKey(prev.ref, prev.pos)) bad = 1;
        if (bad) atomicAdd(&P.res->bad, 1u);
        const bool head = chunkHead(i == 0, prev.ref, prev.bin, v.ref, v.bin);
        const bool tail = v.ref >= 0 && (i + 1 == n || next.ref != v.ref || next.bin != v.bin);
        P.ref[i] = v.ref;
        P.bin[i] = v.bin;
        P.beg[i] = v.pos;
        P.end[i] = (int32_t)v.end;
        P.head[i] = head;
        P.tail[i] = tail;
        if (v.ref >= 0) {
            P.vbeg[i] = voffFixed(streamOffset, coff, start[i], start[n]);
            P.vend[i] = voffFixed(streamOffset, coff, start[i + 1], start[n]);
            if (i == 0 || prev.ref != v.ref) P.info[v.ref].first = (uint32_t)i;
            if (i + 1 == n || next.ref != v.ref) P.info[v.ref].last = (uint32_t)i;
        } else if (i == 0 || prev.ref >= 0) {
            atomicMin(&P.res->noCoorFirst, (uint32_t)i);   // one record of a sorted stream gets here
        }
        sRef[t] = v.ref;
        sEnd[t] = (int32_t)v.end;
        sUnmapped[t] = (v.flag & 4) ? 1u : 0u;
    } else if (i == n) {
        P.head[n] = 0;
    }
    __syncthreads();
    // one atomic per run of a reference in this workgroup, not one per record
    if (sRef[t] >= 0 && (t == 0 || sRef[t - 1] != sRef[t])) {
        const int32_t r = sRef[t];
        int32_t maxEnd = 0;
        uint32_t all = 0, unmapped = 0;
        for (uint32_t k = t; k < kThreads && sRef[k] == r; k++) {
            maxEnd = max(maxEnd, sEnd[k]);
            unmapped += sUnmapped[k];
            all++;
        }
        atomicMax(&P.info[r].maxEnd, maxEnd);
        atomicAdd(&P.info[r].mapped, all - unmapped);
        if (unmapped) atomicAdd(&P.info[r].unmapped, unmapped);
    }
}

__global__ __launch_bounds__(kThreads) void bai_chunk_kernel(uint64_t n, Ptrs P) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t nChunks = P.headIdx[n];
    if (i == 0) P.res->nChunks = nChunks;
    if (i >= nChunks) {
        P.key[i] = kChunkKeyPad;
        P.val[i] = (uint32_t)i;
    }
    const uint32_t before = P.headIdx[i], head = P.head[i];
    if (head) {
        P.key[before] = chunkKey(P.ref[i], P.bin[i]);
        P.val[before] = before;
        P.cbeg[before] = P.vbeg[i];
    }
    if (P.tail[i] && before + head > 0) P.cend[before + head - 1] = P.vend[i];
}

__global__ __launch_bounds__(kThreads) void bai_bin_head_kernel(uint64_t n, Ptrs P) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j > n) return;
    const uint32_t nChunks = P.headIdx[n];
    P.binHead[j] = j < nChunks && (j == 0 || P.keySorted[j - 1] != P.keySorted[j]);
}

__global__ __launch_bounds__(kThreads) void bai_segment_kernel(uint64_t n, uint32_t nRef, Ptrs P) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t nChunks = P.headIdx[n];
    if (j == 0) P.res->nBins = P.binIdx[n];
    if (j >= nChunks) return;
    const uint64_t key = P.keySorted[j];
    const uint32_t r = (uint32_t)(key >> 16);
    if (r >= nRef) return;   // chunk keys come from accepted records
    if (j == 0 || (uint32_t)(P.keySorted[j - 1] >> 16) != r) {
        P.info[r].chunkFirst = (uint32_t)j;
        P.info[r].binFirst = P.binIdx[j];
    }
    if (j + 1 == nChunks || (uint32_t)(P.keySorted[j + 1] >> 16) != r) {
        P.info[r].chunkEnd = (uint32_t)j + 1;
        P.info[r].binEnd = P.binIdx[j + 1];
    }
    if (P.binHead[j]) P.binStart[P.binIdx[j]] = (uint32_t)j;
    if (j + 1 == nChunks) P.binStart[P.binIdx[n]] = nChunks;
}

__device__ bool hasRecords(const RefInfo &I) { return I.mapped + I.unmapped > 0; }
__device__ uint64_t intervals(const RefInfo &I) { return hasRecords(I) ? (uint64_t)lastWindow(I.maxEnd) + 1 : 0; }
__device__ uint64_t bytesOf(const RefInfo &I) {
    return refBytes(hasRecords(I), I.binEnd - I.binFirst, I.chunkEnd - I.chunkFirst, intervals(I));
}

// Inclusive sum over the workgroup's values (kScanThreads of them), through s.
__device__ uint64_t blockInclusive(uint64_t v, uint64_t *s) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const uint64_t r = s[t];
    __syncthreads();
    return r;
}

// Exclusive scans of the references' byte sizes (from the file header on) and interval counts, in
// tiles of one workgroup; check: compare the total with the one already there instead of writing.
__global__ __launch_bounds__(kScanThreads) void bai_ref_scan_kernel(uint32_t nRef, Ptrs P, bool check) {
    __shared__ uint64_t s[kScanThreads];
    uint64_t bytesBefore = kHeaderBytes, linBefore = 0, chunks = 0, bins = 0;
    for (uint32_t r0 = 0; r0 < nRef; r0 += kScanThreads) {
        const uint32_t r = r0 + threadIdx.x;
        RefInfo I{};
        if (r < nRef) I = P.info[r];
        const uint64_t b = r < nRef ? bytesOf(I) : 0, w = r < nRef ? intervals(I) : 0;
        const uint64_t bIn = blockInclusive(b, s), wIn = blockInclusive(w, s);
        const uint64_t cIn = blockInclusive(I.chunkEnd - I.chunkFirst, s), nIn = blockInclusive(I.binEnd - I.binFirst, s);
        if (r < nRef && !check) {
            P.refOff[r] = bytesBefore + bIn - b;
            P.linBase[r] = linBefore + wIn - w;
        }
        // every thread takes the tile's totals from the last one
        if (threadIdx.x == kScanThreads - 1) { s[0] = bIn; s[1] = wIn; s[2] = cIn; s[3] = nIn; }
        __syncthreads();
        bytesBefore += s[0]; linBefore += s[1]; chunks += s[2]; bins += s[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!check) {
            P.refOff[nRef] = bytesBefore;
            P.linBase[nRef] = linBefore;
            P.res->total = bytesBefore + kTrailerBytes;
            P.res->linTotal = linBefore;
        } else if (P.res->total != bytesBefore + kTrailerBytes || P.res->linTotal != linBefore || linBefore > P.linCap ||
                   P.res->nChunks != chunks || P.res->nBins != bins) {
            atomicAdd(&P.res->bad, 1u);
        }
    }
}

__global__ __launch_bounds__(kThreads) void bai_lin_init_kernel(uint32_t nRef, Ptrs P) {
    const uint64_t total = least(P.linBase[nRef], P.linCap);
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < total; k += (uint64_t)gridDim.x * kThreads)
        P.lin[k] = kNoOffset;
}

__global__ __launch_bounds__(kThreads) void bai_lin_kernel(uint64_t n, Ptrs P) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t r = P.ref[i];
    if (r < 0) return;
    const uint32_t w0 = firstWindow(P.beg[i]), w1 = lastWindow(P.end[i]);
    // the record before starts no later: the windows it overlaps already have a smaller offset
    uint32_t w = w0;
    if (i && P.ref[i - 1] == r) {
        const uint32_t prevLast = lastWindow(P.end[i - 1]);
        if (prevLast >= w0) w = prevLast + 1;
    }
    const uint64_t base = P.linBase[r], v = P.vbeg[i];
    for (; w <= w1; w++)
        if (base + w < P.linCap) atomicMin((unsigned long long *)&P.lin[base + w], (unsigned long long)v);
}

// Back-fill: a window nobody overlaps takes the entry of the next overlapped window above it.  One
// workgroup per reference, tiles running downwards with the carry of the tile above.
__global__ __launch_bounds__(kScanThreads) void bai_lin_fill_kernel(Ptrs P) {
    __shared__ uint64_t s[kScanThreads];
    const uint32_t r = blockIdx.x, t = threadIdx.x;
    const uint64_t base = P.linBase[r], count = least(P.linBase[r + 1], P.linCap) - least(base, P.linCap);
    uint64_t carry = kNoOffset;
    for (uint64_t done = 0; done < count; done += kScanThreads) {
        const bool mine = done + t < count;
        const uint64_t at = base + (count - 1 - done - t);   // thread 0 has the tile's highest window
        const uint64_t own = mine ? P.lin[at] : kNoOffset;
        s[t] = own;
        __syncthreads();
        for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
            const uint64_t above = t >= d ? s[t - d] : kNoOffset;
            __syncthreads();
            if (s[t] == kNoOffset) s[t] = above;
            __syncthreads();
        }
        const uint64_t v = s[t] == kNoOffset ? carry : s[t];
        const uint64_t last = s[kScanThreads - 1];
        __syncthreads();
        if (mine && own == kNoOffset) P.lin[at] = v;
        if (last != kNoOffset) carry = last;
    }
}

struct Writer {
    uint32_t *out;
    uint64_t limit;   // the index's bytes, at most the buffer's
    __device__ void u32(uint64_t at, uint32_t v) const {
        if (at + 4 <= limit) out[at / 4] = v;
    }
    __device__ void u64(uint64_t at, uint64_t v) const { u32(at, (uint32_t)v); u32(at + 4, (uint32_t)(v >> 32)); }
};

// Items: sorted chunk j (n of them, the first nChunks real), then reference r, then interval k.
__global__ __launch_bounds__(kThreads) void bai_write_kernel(uint64_t n, uint32_t nRef, Ptrs P, uint8_t *out, uint64_t outCap) {
    const uint64_t item = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const Writer W{(uint32_t *)out, least(P.res->total, outCap)};
    if (item < n) {
        const uint64_t j = item;
        if (j >= P.headIdx[n]) return;
        const uint32_t r = (uint32_t)(P.keySorted[j] >> 16);
        if (r >= nRef) return;
        const RefInfo I = P.info[r];
        const uint32_t head = P.binHead[j], c = P.valSorted[j];
        const uint64_t binsUpToMine = P.binIdx[j] + head - I.binFirst;
        const uint64_t at = P.refOff[r] + 4 + binsUpToMine * 8 + (j - I.chunkFirst) * 16;
        if (head) {
            const uint32_t b = P.binIdx[j];
            W.u32(at - 8, (uint32_t)(P.keySorted[j] & 0xffff));
            W.u32(at - 4, P.binStart[b + 1] - P.binStart[b]);
        }
        W.u64(at, P.cbeg[c]);
        W.u64(at + 8, P.cend[c]);
        return;
    }
    if (item < n + nRef) {
        const uint32_t r = (uint32_t)(item - n);
        const RefInfo I = P.info[r];
        uint64_t at = P.refOff[r];
        if (r == 0) {
            W.u32(0, 0x01494142u);   // "BAI\1"
            W.u32(4, nRef);
        }
        if (r + 1 == nRef) W.u64(P.refOff[nRef], n - least(P.res->noCoorFirst, n));
        if (!hasRecords(I)) {
            W.u32(at, 0);
            W.u32(at + 4, 0);
            return;
        }
        const uint32_t nBins = I.binEnd - I.binFirst, nChunks = I.chunkEnd - I.chunkFirst;
        W.u32(at, nBins + 1);
        at += 4 + (uint64_t)nBins * 8 + (uint64_t)nChunks * 16;
        W.u32(at, kPseudoBin);
        W.u32(at + 4, 2);
        W.u64(at + 8, P.vbeg[I.first]);
        W.u64(at + 16, P.vend[I.last]);
        W.u64(at + 24, I.mapped);
        W.u64(at + 32, I.unmapped);
        W.u32(at + 40, (uint32_t)intervals(I));
        return;
    }
    const uint64_t k = item - n - nRef;
    if (k >= least(P.linBase[nRef], P.linCap)) return;
    // the reference whose intervals hold k: the last r with linBase[r] <= k
    uint32_t lo = 0, hi = nRef;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (P.linBase[mid] <= k) lo = mid; else hi = mid;
    }
    const RefInfo I = P.info[lo];
    const uint64_t at = P.refOff[lo] + 4 + (uint64_t)(I.binEnd - I.binFirst) * 8 + (uint64_t)(I.chunkEnd - I.chunkFirst) * 16 + 44;
    W.u64(at + (k - P.linBase[lo]) * 8, P.lin[k]);
}

// The file without references or records: header and trailer alone.
__global__ void bai_write_empty_kernel(uint64_t n, Ptrs P, uint8_t *out, uint64_t outCap) {
    const Writer W{(uint32_t *)out, least(P.res->total, outCap)};
    W.u32(0, 0x01494142u);
    W.u32(4, 0);
    W.u64(8, n - least(P.res->noCoorFirst, n));
}

__global__ void bai_init_kernel(uint64_t n, Ptrs P) { *P.res = Result{0, 0, 0, 0, 0, (uint32_t)n}; }

inline unsigned blocksFor(uint64_t items) { return (unsigned)((items + kThreads - 1) / kThreads); }

}  // namespace

hipError_t tempBytes(uint64_t n, hipStream_t st, uint64_t *bytes) {
    size_t scan = 0, sort = 0;
    *bytes = 0;
    if (n == 0) return hipSuccess;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n + 1,
                                           rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, sort, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)n, 0u, kChunkKeyBits, st);
    *bytes = scan > sort ? scan : sort;
    return e;
}

Layout layout(uint64_t n, uint64_t nRef, uint64_t temp) {
    Layout L{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at = (at + bytes + 15) & ~15ull;
        return here;
    };
    L.ref = take(n * 4); L.bin = take(n * 4); L.beg = take(n * 4); L.end = take(n * 4);
    L.vbeg = take(n * 8); L.vend = take(n * 8);
    L.head = take((n + 1) * 4); L.tail = take(n * 4); L.headIdx = take((n + 1) * 4);
    L.key = take(n * 8); L.keySorted = take(n * 8); L.val = take(n * 4); L.valSorted = take(n * 4);
    L.cbeg = take(n * 8); L.cend = take(n * 8);
    L.binHead = take((n + 1) * 4); L.binIdx = take((n + 1) * 4); L.binStart = take((n + 1) * 4);
    L.info = take(nRef * sizeof(RefInfo)); L.refOff = take((nRef + 1) * 8); L.linBase = take((nRef + 1) * 8);
    L.linCap = (n < nRef ? n : nRef) * kMaxWindows;
    L.lin = take(L.linCap * 8);
    L.tempBytes = temp;
    L.temp = take(temp);
    L.res = take(sizeof(Result));
    L.bytes = at;
    return L;
}

hipError_t launch(const uint8_t *text, const uint64_t *start, uint64_t n, uint32_t nRef, const uint64_t *coff,
                  uint64_t streamOffset, char *work, const Layout &L, uint8_t *out, uint64_t outCap, hipStream_t st,
                  hipEvent_t *ev) {
    const Ptrs P = carve(work, L);
    auto mark = [&](int k) { return ev ? hipEventRecord(ev[k], st) : hipSuccess; };
    hipError_t e;
#define BAI_TRY(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
    BAI_TRY(mark(0));
    if (nRef) BAI_TRY(hipMemsetAsync(P.info, 0, nRef * sizeof(RefInfo), st));
    hipLaunchKernelGGL(bai_init_kernel, dim3(1), dim3(1), 0, st, n, P);
    size_t temp = L.tempBytes;
    if (n) {
        hipLaunchKernelGGL(bai_field_kernel, dim3(blocksFor(n + 1)), dim3(kThreads), 0, st, text, start, n, nRef, coff,
                           streamOffset, P);
        BAI_TRY(mark(1));
        BAI_TRY(rocprim::exclusive_scan(work + L.temp, temp, P.head, P.headIdx, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(bai_chunk_kernel, dim3(blocksFor(n)), dim3(kThreads), 0, st, n, P);
        BAI_TRY(mark(2));
        temp = L.tempBytes;
        BAI_TRY(rocprim::radix_sort_pairs(work + L.temp, temp, P.key, P.keySorted, P.val, P.valSorted, (size_t)n, 0u,
                                          kChunkKeyBits, st));
        BAI_TRY(mark(3));
        hipLaunchKernelGGL(bai_bin_head_kernel, dim3(blocksFor(n + 1)), dim3(kThreads), 0, st, n, P);
        temp = L.tempBytes;
        BAI_TRY(rocprim::exclusive_scan(work + L.temp, temp, P.binHead, P.binIdx, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(bai_segment_kernel, dim3(blocksFor(n)), dim3(kThreads), 0, st, n, nRef, P);
        BAI_TRY(mark(4));
    } else {
        for (int k = 1; k <= 4; k++) BAI_TRY(mark(k));
    }
    hipLaunchKernelGGL(bai_ref_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, nRef, P, false);
    if (n && nRef) {
        hipLaunchKernelGGL(bai_lin_init_kernel, dim3((unsigned)std::min<uint64_t>(1024, blocksFor(L.linCap))), dim3(kThreads), 0, st, nRef, P);
        hipLaunchKernelGGL(bai_lin_kernel, dim3(blocksFor(n)), dim3(kThreads), 0, st, n, P);
        hipLaunchKernelGGL(bai_lin_fill_kernel, dim3(nRef), dim3(kScanThreads), 0, st, P);
    }
    BAI_TRY(mark(5));
    if (nRef)
        hipLaunchKernelGGL(bai_write_kernel, dim3(blocksFor(n + nRef + L.linCap)), dim3(kThreads), 0, st, n, nRef, P, out, outCap);
    else
        hipLaunchKernelGGL(bai_write_empty_kernel, dim3(1), dim3(1), 0, st, n, P, out, outCap);
    BAI_TRY(mark(6));
    hipLaunchKernelGGL(bai_ref_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, nRef, P, true);
    BAI_TRY(mark(7));
#undef BAI_TRY
    return hipGetLastError();
}

}  // namespace baigpu
