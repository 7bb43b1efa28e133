// dupmark.cpp -- the host model of the device duplicate marking (dupmark.hip):
// snapgpu_bam_mark_duplicates, one serial walk over the records with the rule of dupmark_rule.h, in
// place.  Byte-identical to the device's records; needs no GPU.
#include "internal.h"
#include "dupmark_rule.h"

#include <cstdio>
#include <vector>

using namespace baiindex;
using namespace duprule;

namespace {

int refuse(uint64_t record, const char *why, int code = SNAPGPU_EFORMAT) {
    char msg[160];
    snprintf(msg, sizeof msg, "bam_mark_duplicates: record %llu: %s", (unsigned long long)record, why);
    snapgpu::setError(msg);
    return code;
}

// What the marking keeps of one record.
struct Seen {
    uint64_t at;       // its first byte
    uint64_t key;      // sortKey
    uint32_t score;
    bool considered;
    uint8_t strand;
};

}  // namespace

extern "C" int snapgpu_bam_mark_duplicates(char *records, uint64_t n, int32_t nRef, uint64_t *nMarked, uint64_t *nGroups) {
    if ((!records && n) || !nMarked || !nGroups || nRef < 0) {
        snapgpu::setError("bam_mark_duplicates: bad argument");
        return SNAPGPU_EINVAL;
    }
    *nMarked = *nGroups = 0;
    uint8_t *rec = (uint8_t *)records;
    // the whole stream is read before a byte changes: a refused stream stays as it was
    std::vector<Seen> seen;
    uint64_t prevKey = 0;
    for (uint64_t u = 0, i = 0; u < n; i++) {
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
        prevKey = key;
        if (f.flag & kMateFlag) return refuse(i, "has a mate (FLAG 0x1): the mate rule is not built", SNAPGPU_EINVAL);
        const uint32_t lSeq = seqLen(rec + u);
        if (lSeq > kMaxSeq) return refuse(i, "l_seq above 2^24");
        if (!holdsQual(f, lSeq, bytes)) return refuse(i, "truncated (its QUAL passes its end)");
        if (i >= 0xfffffffeull) return refuse(i, "too many records", SNAPGPU_EINVAL);
        Seen s{u, key, 0, considered(f), (uint8_t)strand(f.flag)};
        if (s.considered) {
            const uint8_t *q = rec + u + qualOffset(f, lSeq);
            for (uint32_t k = 0; k < lSeq; k++) s.score += qualValue(q[k]);
        }
        seen.push_back(s);
        u += bytes;
    }
    for (size_t i = 0; i < seen.size();) {
        // the records of one location: its two strands are two groups
        size_t j = i;
        uint64_t best[2] = {0, 0}, size[2] = {0, 0};
        for (; j < seen.size() && seen[j].key == seen[i].key; j++) {
            const Seen &s = seen[j];
            if (!s.considered) continue;
            const uint64_t r = rank(s.score, (uint32_t)j);
            if (r > best[s.strand]) best[s.strand] = r;
            size[s.strand]++;
        }
        for (size_t k = i; k < j; k++) {
            const Seen &s = seen[k];
            const bool marked = s.considered && rank(s.score, (uint32_t)k) != best[s.strand];
            uint8_t *b = rec + s.at + kFlagHighByte;
            *b = flagByte(*b, marked);
            *nMarked += marked;
        }
        for (int s = 0; s < 2; s++) *nGroups += size[s] >= 2;
        i = j;
    }
    return SNAPGPU_OK;
}
