// bai.cpp -- the host model of the device BAI builder (bai.hip): snapgpu_bai_build, one serial walk
// over the records with the rules of bai_index.h.  Byte-identical to the device index; needs no GPU.
#include "internal.h"
#include "bai_index.h"
#include "inflate_block.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

using namespace baiindex;

namespace {

int refuse(uint64_t record, const char *why) {
    char msg[160];
    snprintf(msg, sizeof msg, "bai_build: record %llu: %s", (unsigned long long)record, why);
    snapgpu::setError(msg);
    return SNAPGPU_EFORMAT;
}

// Virtual offsets over any member table: the member that holds byte u, or, at the end of the data,
// where the members that hold nothing (an EOF block) begin.
struct Members {
    std::vector<uint64_t> uEnd, cStart;   // uEnd[m]: bytes up to and including member m; cStart[m], cStart[nMembers]
    uint64_t streamOffset = 0, dataEnd = 0;
    uint64_t at(uint64_t u) const {
        const size_t m = std::upper_bound(uEnd.begin(), uEnd.end(), u) - uEnd.begin();
        if (m == uEnd.size()) return voff(streamOffset, dataEnd, 0);
        return voff(streamOffset, cStart[m], (uint32_t)(u - (m ? uEnd[m - 1] : 0)));
    }
};

struct Out {
    std::vector<unsigned char> b;
    void u32(uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((unsigned char)(v >> (8 * k))); }
    void u64(uint64_t v) { u32((uint32_t)v); u32((uint32_t)(v >> 32)); }
};

struct Chunk { uint64_t beg, end; };

}  // namespace

extern "C" uint64_t snapgpu_bai_size_bound(uint64_t nRecords, uint64_t nRef, uint64_t recordBytes) {
    return sizeBound(nRecords, nRef, recordBytes);
}

extern "C" int snapgpu_bai_build(const char *records, uint64_t n, int32_t nRef, const char *bgzf, uint64_t bgzfBytes,
                                 uint64_t streamOffset, char *out, uint64_t cap, uint64_t *used) {
    if ((!records && n) || (!bgzf && bgzfBytes) || !used || nRef < 0) {
        snapgpu::setError("bai_build: bad argument");
        return SNAPGPU_EINVAL;
    }
    if (streamOffset >= kStreamOffsetLimit) {
        snapgpu::setError("bai_build: streamOffset does not fit a virtual offset");
        return SNAPGPU_EINVAL;
    }
    *used = 0;
    std::vector<inflateblock::Member> members;
    uint64_t inflated = 0;
    if (int rc = snapgpu::bgzfWalk("bai_build", bgzf, bgzfBytes, members, &inflated)) return rc;
    if (inflated != n) {
        snapgpu::setError("bai_build: the members' ISIZEs do not sum to the records' bytes");
        return SNAPGPU_EINVAL;
    }
    Members M;
    M.streamOffset = streamOffset;
    M.dataEnd = bgzfBytes;
    for (size_t m = members.size(); m > 0 && members[m - 1].outSize == 0; m--) M.dataEnd = members[m - 1].inStart;
    for (const auto &m : members) {
        M.uEnd.push_back(m.outStart + m.outSize);
        M.cStart.push_back(m.inStart);
    }

    const uint8_t *rec = (const uint8_t *)records;
    Out O;
    O.b.reserve(4096);
    O.u32(0x01494142u);   // "BAI\1"
    O.u32((uint32_t)nRef);
    uint64_t u = 0, i = 0, prevKey = 0, noCoor = 0;
    int32_t nextRef = 0;   // references below it are written
    auto emptyRefs = [&](int32_t upTo) {
        for (; nextRef < upTo; nextRef++) { O.u32(0); O.u32(0); }
    };
    while (u < n) {
        // one reference's records, or the records without one
        std::map<uint32_t, std::vector<Chunk>> bins;
        std::vector<uint64_t> lin;
        uint64_t mapped = 0, unmapped = 0, firstBeg = 0, lastEnd = 0;
        int32_t ref = -2, prevRef = -2;
        uint32_t prevBin = 0;
        bool first = true;
        while (u < n) {
            if (n - u < 4) return refuse(i, "truncated");
            const uint64_t bytes = (uint64_t)load32(rec + u) + 4;
            if (bytes < kFixed || bytes > n - u) return refuse(i, "truncated");
            const Fields f = fields(rec + u);
            if (!holdsCigar(f, bytes)) return refuse(i, "truncated (its CIGAR passes its end)");
            const int64_t end = (int64_t)f.pos + span(rec + u, f);
            switch (refusal(f, end, nRef)) {
            case kBadRef: return refuse(i, "refID outside [-1, nRef)");
            case kBadPos: return refuse(i, "pos < 0 with a refID");
            case kBadEnd: return refuse(i, "ends past 2^29");
            default: break;
            }
            const uint64_t key = sortKey(f.refID, f.pos);
            if (i && key < prevKey) return refuse(i, "not in (refID, pos) order");
            if (!first && f.refID != ref) break;   // the next reference's first record: not consumed
            prevKey = key;
            ref = f.refID;
            if (ref < 0) {
                noCoor++;
            } else {
                const uint64_t vb = M.at(u), ve = M.at(u + bytes);
                if (chunkHead(first, prevRef, prevBin, ref, f.bin)) bins[f.bin].push_back(Chunk{vb, ve});
                else bins[f.bin].back().end = ve;
                if (first) firstBeg = vb;
                lastEnd = ve;
                (f.flag & 4 ? unmapped : mapped)++;
                const uint32_t w0 = firstWindow(f.pos), w1 = lastWindow(end);
                if (lin.size() <= w1) lin.resize(w1 + 1, kNoOffset);
                for (uint32_t w = w0; w <= w1; w++) lin[w] = std::min(lin[w], vb);
            }
            prevRef = ref;
            prevBin = f.bin;
            first = false;
            u += bytes;
            i++;
        }
        if (ref < 0) continue;
        emptyRefs(ref);
        nextRef = ref + 1;
        uint64_t nChunks = 0;
        for (const auto &b : bins) nChunks += b.second.size();
        const size_t before = O.b.size();
        O.u32((uint32_t)bins.size() + 1);
        for (const auto &b : bins) {
            O.u32(b.first);
            O.u32((uint32_t)b.second.size());
            for (const Chunk &c : b.second) { O.u64(c.beg); O.u64(c.end); }
        }
        O.u32(kPseudoBin);
        O.u32(2);
        O.u64(firstBeg); O.u64(lastEnd); O.u64(mapped); O.u64(unmapped);
        O.u32((uint32_t)lin.size());
        for (size_t w = lin.size(); w-- > 0;)   // htslib's back-fill
            if (lin[w] == kNoOffset) lin[w] = lin[w + 1];
        for (uint64_t v : lin) O.u64(v);
        if (O.b.size() - before != refBytes(true, bins.size(), nChunks, lin.size())) {
            snapgpu::setError("bai_build: a reference's bytes are not what its counts give");
            return SNAPGPU_EIO;
        }
    }
    emptyRefs(nRef);
    O.u64(noCoor);
    *used = O.b.size();
    if (O.b.size() > cap || !out) {
        snapgpu::setError("bai_build: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    memcpy(out, O.b.data(), O.b.size());
    return SNAPGPU_OK;
}
