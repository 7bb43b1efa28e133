// bai_model_test.cpp -- snapgpu_bai_build (snap-rnaseq_amd/csrc/host/bai.cpp over csrc/bai_index.h, the
// rules the device passes compile) as a stand-alone program: built from the host sources with
// -fsanitize=address,undefined, every buffer exactly as long as its contents, so a read outside the
// records or the members, or a write outside the index, is an error here.
//
// Seeded random streams of BAM records in (refID, pos) order -- mixed name, CIGAR and sequence
// lengths, records that cross members, empty references, records without a reference -- are
// compressed by snapgpu_bgzf_compress_model and indexed into a buffer of exactly the size the first
// call reports.  Each stream is then cut at a random byte: the cut form is refused with
// SNAPGPU_EFORMAT unless the cut falls between two records.
//
//   bai_model_test [random cases]
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

uint64_t g_state = 0x853c49e6748fea9bull;
uint32_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int g_failed = 0, g_built = 0, g_refused = 0;
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
    explicit Exact(size_t size) : p(new unsigned char[size ? size : 1]), n(size) {}
    ~Exact() { delete[] p; }
    Exact(const Exact &) = delete;
    const char *c() const { return n ? (const char *)p : nullptr; }
};

// One random stream -> its bytes, the record starts, the records without a reference.
void makeStream(Bytes &s, std::vector<size_t> &starts, int32_t &nRef, uint64_t &noCoor) {
    static const uint32_t ops[] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    nRef = 1 + (int32_t)(rnd() % 4);
    noCoor = 0;
    const uint32_t nRec = rnd() % 8 == 0 ? 0 : rnd() % 60;
    int32_t ref = rnd() % 3 == 0 ? (int32_t)(rnd() % nRef) : 0, pos = (int32_t)(rnd() % 40000);
    for (uint32_t i = 0; i < nRec; i++) {
        if (ref >= 0) {
            const uint32_t step = rnd() % 10;
            if (step == 0) { ref++; pos = (int32_t)(rnd() % 100000); }
            else if (step < 4) pos += (int32_t)(rnd() % 50000);
            else if (step < 8) pos += (int32_t)(rnd() % 200);
            if (ref >= nRef || (i + 3 > nRec && rnd() % 2)) ref = -1;
        }
        const uint32_t nameLen = 1 + rnd() % 20, nOps = rnd() % 5;
        const uint32_t lSeq = rnd() % 20 == 0 ? rnd() % 50000 : rnd() % 300;
        uint32_t cigar[4];
        for (uint32_t k = 0; k < nOps; k++) {
            const uint32_t op = ops[rnd() % 9], len = rnd() % 16 == 0 ? rnd() % 60000 : 1 + rnd() % 150;
            cigar[k] = len << 4 | op;
        }
        starts.push_back(s.size());
        put32(s, 32 + nameLen + 4 * nOps + (lSeq + 1) / 2 + lSeq);
        put32(s, (uint32_t)ref);
        put32(s, (uint32_t)(ref < 0 ? -1 : pos));
        s.push_back((unsigned char)nameLen);
        s.push_back(30);
        put16(s, 4681 + rnd() % 40);     // the index takes the record's own bin, whatever it is
        put16(s, nOps);
        put16(s, rnd() % 4 == 0 ? 4 : 0);
        put32(s, lSeq);
        put32(s, 0xffffffffu); put32(s, 0xffffffffu); put32(s, 0);
        for (uint32_t k = 0; k + 1 < nameLen; k++) s.push_back('a' + k % 26);
        s.push_back(0);
        for (uint32_t k = 0; k < nOps; k++) put32(s, cigar[k]);
        for (uint32_t k = 0; k < (lSeq + 1) / 2 + lSeq; k++) s.push_back((unsigned char)(rnd() % 7 == 0 ? rnd() : 0x11));
        if (ref < 0) noCoor++;
    }
}

// snapgpu_bgzf_compress_model into a block of exactly its size
Exact *compress(const Exact &in, int eof) {
    uint64_t used = 0;
    snapgpu_bgzf_compress_model(in.c(), in.n, eof, nullptr, 0, &used);
    Exact *z = new Exact((size_t)used);
    if (snapgpu_bgzf_compress_model(in.c(), in.n, eof, (char *)z->p, used, &used) != SNAPGPU_OK || used != z->n) {
        delete z;
        return nullptr;
    }
    return z;
}

uint32_t get32(const unsigned char *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

void oneCase(int c) {
    Bytes s;
    std::vector<size_t> starts;
    int32_t nRef;
    uint64_t noCoor;
    makeStream(s, starts, nRef, noCoor);
    const uint64_t offset = rnd() % 2 ? 0 : rnd();
    {
        const Exact rec(s);
        Exact *z = compress(rec, (int)(rnd() % 2));
        if (!z) return fail("compress", c);
        uint64_t need = 0, used = 0;
        const int rc0 = snapgpu_bai_build(rec.c(), rec.n, nRef, z->c(), z->n, offset, nullptr, 0, &need);
        if (rc0 != SNAPGPU_EINVAL || need < 16 || need > snapgpu_bai_size_bound(starts.size(), (uint64_t)nRef, rec.n)) {
            delete z;
            return fail("size query", c);
        }
        Exact out((size_t)need);
        const int rc = snapgpu_bai_build(rec.c(), rec.n, nRef, z->c(), z->n, offset, (char *)out.p, need, &used);
        delete z;
        if (rc != SNAPGPU_OK || used != need) return fail("build", c);
        if (memcmp(out.p, "BAI\1", 4) || get32(out.p + 4) != (uint32_t)nRef || get32(out.p + need - 8) != noCoor ||
            get32(out.p + need - 4) != 0)
            return fail("header or trailer", c);
        g_built++;
    }
    if (s.empty()) return;
    const size_t cut = rnd() % s.size();
    bool boundary = false;
    for (size_t k = 0; k < starts.size(); k++)
        if (starts[k] == cut) boundary = true;
    Bytes t(s.begin(), s.begin() + cut);
    const Exact rec(t);
    Exact *z = compress(rec, 1);
    if (!z) return fail("compress (cut)", c);
    uint64_t need = 0;
    const int rc = snapgpu_bai_build(rec.c(), rec.n, nRef, z->c(), z->n, offset, nullptr, 0, &need);
    delete z;
    if (boundary ? rc != SNAPGPU_EINVAL || need < 16 : rc != SNAPGPU_EFORMAT) return fail("cut form", c);
    if (!boundary) g_refused++;
}

}  // namespace

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 2000;
    for (int c = 0; c < n; c++) oneCase(c);
    printf("%d streams indexed, %d truncated forms refused, %d failed\n", g_built, g_refused, g_failed);
    return g_failed ? 1 : 0;
}
