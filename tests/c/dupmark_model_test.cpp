// dupmark_model_test.cpp -- snapgpu_bam_mark_duplicates (snap-rnaseq_amd/csrc/host/dupmark.cpp over
// csrc/dupmark_rule.h, the rule the device passes compile) as a stand-alone program: built from the host
// source with -fsanitize=address,undefined, every stream in a heap block of exactly its size, so a read or
// a write outside the records is an error here.
//
// Seeded random streams of single-end BAM records in (refID, pos) order over few distinct positions --
// mixed name, CIGAR and sequence lengths, both strands, placed and unplaced unmapped records, stray 0x400
// bits -- are marked in place.  Checked without the model's code: nothing but bit 0x04 of byte 19 differs,
// every group keeps exactly one record and it is the first of the highest score, records outside the
// groups carry no mark, the counts are those of the bytes, a second call changes nothing.  Each stream is
// then cut at a random byte: the cut form is refused with SNAPGPU_EFORMAT and left as it was, unless the
// cut falls between two records.
//
//   dupmark_model_test [random cases]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "snapgpu.h"

namespace snapgpu {
void setError(const std::string &) {}
}

namespace {

typedef std::vector<unsigned char> Bytes;

uint64_t g_state = 0x2545f4914f6cdd1dull;
uint32_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int g_failed = 0, g_marked = 0, g_refused = 0;
void fail(const char *what, int c) {
    if (g_failed++ < 20) printf("FAIL %s (case %d)\n", what, c);
}

void put16(Bytes &b, uint32_t v) { b.push_back((unsigned char)v); b.push_back((unsigned char)(v >> 8)); }
void put32(Bytes &b, uint32_t v) { put16(b, v & 0xffffu); put16(b, v >> 16); }

// a copy in a heap block of exactly the bytes' size
struct Exact {
    unsigned char *p;
    size_t n;
    explicit Exact(const Bytes &b) : p(new unsigned char[b.size() ? b.size() : 1]), n(b.size()) {
        if (n) memcpy(p, b.data(), n);
    }
    ~Exact() { delete[] p; }
    Exact(const Exact &) = delete;
    char *c() const { return n ? (char *)p : nullptr; }
};

struct Rec {
    size_t at;
    int32_t ref, pos;
    uint32_t flag, score, lSeq;
    size_t qualAt;
};

void makeStream(Bytes &s, std::vector<Rec> &recs, int32_t &nRef) {
    nRef = 1 + (int32_t)(rnd() % 3);
    const uint32_t nRec = rnd() % 8 == 0 ? 0 : rnd() % 80;
    int32_t ref = 0, pos = (int32_t)(rnd() % 50);
    for (uint32_t i = 0; i < nRec; i++) {
        if (ref >= 0) {
            const uint32_t step = rnd() % 10;
            if (step == 0) { ref++; pos = (int32_t)(rnd() % 10); }
            else if (step < 4) pos += (int32_t)(1 + rnd() % 3);
            if (ref >= nRef || (i + 4 > nRec && rnd() % 2)) ref = -1;
        }
        const uint32_t nameLen = 1 + rnd() % 20, nOps = rnd() % 4;
        const uint32_t lSeq = rnd() % 25 == 0 ? rnd() % 5000 : rnd() % 12 == 0 ? 0 : rnd() % 120;
        uint32_t flag = (rnd() % 3 == 0 ? 0x10u : 0u) | (rnd() % 5 == 0 ? 0x400u : 0u) | (rnd() % 9 == 0 ? 0x100u : 0u);
        if (ref < 0 || rnd() % 10 == 0) flag |= 4;
        Rec r{s.size(), ref, ref < 0 ? -1 : pos, flag, 0, lSeq, 0};
        put32(s, 32 + nameLen + 4 * nOps + (lSeq + 1) / 2 + lSeq);
        put32(s, (uint32_t)r.ref);
        put32(s, (uint32_t)r.pos);
        s.push_back((unsigned char)nameLen);
        s.push_back(30);
        put16(s, 4681);
        put16(s, nOps);
        put16(s, flag);
        put32(s, lSeq);
        put32(s, 0xffffffffu); put32(s, 0xffffffffu); put32(s, 0);
        for (uint32_t k = 0; k + 1 < nameLen; k++) s.push_back('a' + k % 26);
        s.push_back(0);
        for (uint32_t k = 0; k < nOps; k++) put32(s, (1 + rnd() % 100) << 4 | (rnd() % 9));
        for (uint32_t k = 0; k < (lSeq + 1) / 2; k++) s.push_back((unsigned char)rnd());
        r.qualAt = s.size();
        const uint32_t kind = rnd() % 4;   // narrow ranges make ties; 0xff counts 0
        for (uint32_t k = 0; k < lSeq; k++) {
            const unsigned char q = kind == 0 ? 30 : kind == 1 ? (unsigned char)(rnd() % 3 ? 0xff : 0) : (unsigned char)(rnd() % 256);
            s.push_back(q);
            r.score += q == 0xff ? 0 : q;
        }
        recs.push_back(r);
    }
}

bool isConsidered(const Rec &r) { return r.ref >= 0 && r.pos >= 0 && !(r.flag & 4); }

void oneCase(int c) {
    Bytes s;
    std::vector<Rec> recs;
    int32_t nRef;
    makeStream(s, recs, nRef);
    {
        const Exact buf(s);
        uint64_t marked = 99, groups = 99;
        if (snapgpu_bam_mark_duplicates(buf.c(), buf.n, nRef, &marked, &groups) != SNAPGPU_OK) return fail("mark", c);
        uint64_t seenMarked = 0, seenGroups = 0;
        for (size_t k = 0; k < s.size(); k++)
            if (buf.p[k] != s[k]) {
                bool flagByte = false;
                for (const Rec &r : recs) flagByte |= k == r.at + 19;
                if (!flagByte || ((buf.p[k] ^ s[k]) & ~0x04)) return fail("a byte other than 0x400's changed", c);
            }
        for (size_t i = 0; i < recs.size(); i++) {
            const Rec &r = recs[i];
            const bool dup = buf.p[r.at + 19] & 0x04;
            seenMarked += dup;
            if (!isConsidered(r)) {
                if (dup) return fail("a mark outside the groups", c);
                continue;
            }
            // the kept one of r's group: the first of the highest score
            size_t kept = i, size = 0, first = i;
            bool have = false;
            for (size_t j = 0; j < recs.size(); j++) {
                const Rec &o = recs[j];
                if (!isConsidered(o) || o.ref != r.ref || o.pos != r.pos || (o.flag & 0x10) != (r.flag & 0x10)) continue;
                if (!have) first = j;
                if (!have || o.score > recs[kept].score) kept = j;
                have = true;
                size++;
            }
            if (dup != (kept != i)) return fail("the kept record", c);
            if (first == i && size >= 2) seenGroups++;
        }
        if (marked != seenMarked || groups != seenGroups) return fail("counts", c);
        const Bytes once(buf.p, buf.p + buf.n);
        if (snapgpu_bam_mark_duplicates(buf.c(), buf.n, nRef, &marked, &groups) != SNAPGPU_OK || marked != seenMarked ||
            groups != seenGroups || (buf.n && memcmp(buf.p, once.data(), buf.n)))
            return fail("second application", c);
        g_marked++;
    }
    if (s.empty()) return;
    const size_t cut = rnd() % s.size();
    bool boundary = false;
    for (const Rec &r : recs)
        if (r.at == cut) boundary = true;
    const Bytes t(s.begin(), s.begin() + cut);
    const Exact buf(t);
    uint64_t marked = 0, groups = 0;
    const int rc = snapgpu_bam_mark_duplicates(buf.c(), buf.n, nRef, &marked, &groups);
    if (boundary ? rc != SNAPGPU_OK : rc != SNAPGPU_EFORMAT || (buf.n && memcmp(buf.p, t.data(), buf.n))) return fail("cut form", c);
    if (!boundary) g_refused++;
}

}  // namespace

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 2000;
    for (int c = 0; c < n; c++) oneCase(c);
    printf("%d streams marked, %d truncated forms refused, %d failed\n", g_marked, g_refused, g_failed);
    return g_failed ? 1 : 0;
}
