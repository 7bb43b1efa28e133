// sam_pair_line_test.cpp -- csrc/sam_pair_line.h with the Serial group in a program of its own, to be
// built with -fsanitize=address,undefined: seeded random pair batches whose every array lives in a
// heap block of exactly its size (reads, qualities and ids back to back without slack, the text
// buffer of exactly the summed line lengths), so a read or a store one byte outside is reported.
// Every line must end where its length says, carry the right number of tabs, and give back the
// fields pairFields() decided when it is parsed again.
//
//   sam_pair_line_test [batches]
#include "sam_pair_line.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t n) {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a heap block of exactly v's size
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

struct End {
    std::vector<char> bases, quals, ids;
    std::vector<uint64_t> offsets, idOffsets;
    std::vector<uint32_t> lengths, front, unclipped, idLengths;
};

int failures = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (failures++ < 10) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

uint64_t lines = 0;

void oneBatch(uint32_t n, bool clippedBatch, bool withRg) {
    const uint32_t pieceOffsets[3] = {500, 70000, 200000};
    const char names[] = "chr1chromosome_twoX";
    const uint32_t nameOff[4] = {0, 4, 18, 19};
    End E[2];
    std::vector<snapgpu_pair_result_t> res(n);
    std::vector<int32_t> ed(2 * n);
    std::vector<uint32_t> nOps(2 * n), ops(2 * (size_t)n * SNAPGPU_CIGAR_MAX_OPS);
    for (uint32_t q = 0; q < n; q++) {
        snapgpu_pair_result_t &r = res[q];
        memset(&r, 0, sizeof(r));
        const uint32_t idKind = rnd(6);
        for (int e = 0; e < 2; e++) {
            End &X = E[e];
            const uint32_t full = 50 + rnd(rnd(8) == 0 ? 975 : 120);   // up to 1024
            uint32_t front = 0, back = 0;
            if (clippedBatch && rnd(2)) { front = rnd(6); back = rnd(8); }
            X.offsets.push_back(X.bases.size() + front);
            X.lengths.push_back(full - front - back);
            X.front.push_back(front);
            X.unclipped.push_back(full);
            for (uint32_t k = 0; k < full; k++) {
                const uint32_t c = rnd(400);
                X.bases.push_back(c == 0 ? 'R' : c == 1 ? 0 : "ACGTacgtNn"[c % 10]);
                X.quals.push_back(c == 2 ? 0 : (char)('!' + rnd(60)));
            }
            std::string id = "pair" + std::to_string(q);
            if (idKind == 1 && e) id += "longer";
            if (idKind == 2) id += " comment";
            if (idKind == 3) id = "";
            if (idKind != 4) id += e == (idKind == 5 ? 1 : 0) ? "/1" : "/2";
            if (idKind == 4) id += "/1";
            X.idOffsets.push_back(X.ids.size());
            X.idLengths.push_back((uint32_t)id.size());
            X.ids.insert(X.ids.end(), id.begin(), id.end());
            const uint32_t kind = rnd(8);
            r.status[e] = kind == 0 ? SNAPGPU_NOT_FOUND : kind == 1 ? SNAPGPU_MULTIPLE_HITS : SNAPGPU_SINGLE_HIT;
            r.location[e] = kind == 2 ? samline::kInvalid : kind == 3 ? rnd(500) : 500 + rnd(299000);
            if (e && rnd(10) == 0) r.location[1] = r.location[0];
            r.direction[e] = (uint8_t)rnd(2);
            r.mapq[e] = (int32_t)rnd(120) - 20;
            const uint64_t row = 2ull * q + e;
            ed[row] = (int32_t)rnd(40) - 5;
            nOps[row] = rnd(SNAPGPU_CIGAR_MAX_OPS + 1);
            for (uint32_t k = 0; k < SNAPGPU_CIGAR_MAX_OPS; k++) ops[row * SNAPGPU_CIGAR_MAX_OPS + k] = (rnd(1200) + 1) << 4 | rnd(9);
        }
    }
    samline::PairArgs A;
    memset(&A, 0, sizeof(A));
    std::unique_ptr<char[]> hold[6];
    std::unique_ptr<uint64_t[]> hold64[4];
    std::unique_ptr<uint32_t[]> hold32[8];
    for (int e = 0; e < 2; e++) {
        A.bases[e] = (hold[3 * e] = exact(E[e].bases)).get();
        A.quals[e] = (hold[3 * e + 1] = exact(E[e].quals)).get();
        A.ids[e] = (hold[3 * e + 2] = exact(E[e].ids)).get();
        A.offsets[e] = (hold64[2 * e] = exact(E[e].offsets)).get();
        A.idOffsets[e] = (hold64[2 * e + 1] = exact(E[e].idOffsets)).get();
        A.lengths[e] = (hold32[4 * e] = exact(E[e].lengths)).get();
        A.idLengths[e] = (hold32[4 * e + 1] = exact(E[e].idLengths)).get();
        if (clippedBatch) {
            A.front[e] = (hold32[4 * e + 2] = exact(E[e].front)).get();
            A.unclipped[e] = (hold32[4 * e + 3] = exact(E[e].unclipped)).get();
        } else {   // an unclipped batch: the reads are their whole extents
            for (uint32_t q = 0; q < n; q++) { E[e].offsets[q] -= E[e].front[q]; E[e].lengths[q] = E[e].unclipped[q]; }
            A.offsets[e] = (hold64[2 * e] = exact(E[e].offsets)).get();
            A.lengths[e] = (hold32[4 * e] = exact(E[e].lengths)).get();
        }
    }
    auto hRes = exact(res);
    auto hEd = exact(ed);
    auto hN = exact(nOps), hOps = exact(ops);
    A.res = hRes.get(); A.ed = hEd.get(); A.nOps = hN.get(); A.ops = hOps.get();
    A.rowPair = 2; A.rowEnd = 1;
    A.pieceOffsets = pieceOffsets; A.pieceNameOff = nameOff; A.pieceNames = names; A.nPieces = 3;
    const std::string rg = std::string(rnd(40), 'g');
    A.rg = withRg ? rg.c_str() : nullptr;
    A.rgLen = withRg ? (uint32_t)rg.size() : 0;

    const samline::Serial none{nullptr};
    std::vector<uint32_t> len(2 * n);
    uint64_t total = 0;
    for (uint64_t j = 0; j < 2ull * n; j++) total += len[j] = samline::pairLineLength(A, samline::pairFields(A, j, none));
    std::unique_ptr<char[]> out(new char[total]);
    memset(out.get(), 0x7f, total);
    const samline::Serial g{out.get()};
    uint64_t at = 0;
    for (uint64_t j = 0; j < 2ull * n; j++) {
        const samline::PairFields P = samline::pairFields(A, j, g);
        // the device write pass hands the length pass's scans back in: the same fields either way
        const samline::Scans known{P.F.qlen, (uint16_t)P.F.seqLen, (uint16_t)P.F.qualLen};
        const samline::PairFields K = samline::pairFields(A, j, g, &known);
        CHECK(samline::pairLineLength(A, K) == len[j], "record %llu: length with scans", (unsigned long long)j);
        samline::pairWrite(A, j, K, at, g);
        const char *l = out.get() + at;
        CHECK(l[len[j] - 1] == '\n', "record %llu does not end in a newline", (unsigned long long)j);
        std::vector<std::string> f(1);
        for (uint32_t k = 0; k + 1 < len[j]; k++) {
            CHECK(l[k] != 0x7f && l[k] != '\n', "record %llu: byte %u not written", (unsigned long long)j, k);
            if (l[k] == '\t') f.emplace_back(); else f.back() += l[k];
        }
        CHECK(f.size() == (withRg ? 14u : 13u), "record %llu has %zu fields", (unsigned long long)j, f.size());
        if (f.size() >= 13) {
            CHECK(f[1] == std::to_string(P.F.flags) && f[3] == std::to_string(P.F.pos) && f[4] == std::to_string(P.F.mapq),
                  "record %llu: FLAG / POS / MAPQ", (unsigned long long)j);
            CHECK(f[7] == std::to_string(P.pnext) && f[8] == std::to_string((long long)P.tlen), "record %llu: PNEXT / TLEN",
                  (unsigned long long)j);
            CHECK(f[9].size() == P.F.seqLen && f[10].size() == P.F.qualLen, "record %llu: SEQ / QUAL", (unsigned long long)j);
            CHECK(f.back() == "NM:i:" + std::to_string(P.F.ed), "record %llu: NM", (unsigned long long)j);
            const bool w = j & 1;
            CHECK((P.F.flags & 0xc1) == (w ? 0x81u : 0x41u), "record %llu: segment flags", (unsigned long long)j);
            if (P.F.flags & 0x4) CHECK(f[5] == "*" && P.F.ed == -1, "record %llu: unmapped", (unsigned long long)j);
        }
        at += len[j];
        lines++;
    }
    CHECK(at == total, "the lines do not fill the buffer");
}

}  // namespace

int main(int argc, char **argv) {
    const int batches = argc > 1 ? atoi(argv[1]) : 200;
    for (int b = 0; b < batches; b++) oneBatch(1 + rnd(40), b & 1, (b & 2) != 0);
    printf("%d batches, %llu lines, %d failed\n", batches, (unsigned long long)lines, failures);
    return failures ? 1 : 0;
}
