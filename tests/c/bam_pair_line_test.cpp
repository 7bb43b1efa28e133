// bam_pair_line_test.cpp -- csrc/bam_pair_line.h with the Serial group in a program of its own, to be
// built with -fsanitize=address,undefined: seeded random pair batches whose every array lives in a
// heap block of exactly its size (reads, qualities and ids back to back without slack), written into a
// record buffer of exactly the summed record sizes between two rows of guard bytes, so a read or a
// store one byte outside is reported.  Every record must carry the block_size its length says, fill
// every byte of it, and give back the fields fields() decided when it is parsed again; the NM values
// follow the carry rule, and the sort key is getSortInfo's.
//
//   bam_pair_line_test [batches]
#include "bam_pair_line.h"

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

uint64_t records = 0, carried = 0;
constexpr uint32_t kGuard = 64;

uint32_t get32(const char *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
uint32_t get16(const char *p) {
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}

void oneBatch(uint32_t n, bool clippedBatch, bool withRg) {
    const uint32_t pieceOffsets[3] = {500, 70000, 200000};
    End E[2];
    std::vector<snapgpu_pair_result_t> res(n);
    std::vector<int32_t> ed(2 * n);
    std::vector<uint32_t> nOps(2 * n), ops(2 * (size_t)n * SNAPGPU_CIGAR_MAX_OPS);
    for (uint32_t q = 0; q < n; q++) {
        snapgpu_pair_result_t &r = res[q];
        memset(&r, 0, sizeof(r));
        const uint32_t idKind = rnd(7), longKind = rnd(2);
        for (int e = 0; e < 2; e++) {
            End &X = E[e];
            const uint32_t full = 1 + rnd(rnd(8) == 0 ? 1024 : 170);   // 1 .. 1024, odd and even
            uint32_t front = 0, back = 0;
            if (clippedBatch && rnd(2) && full > 16) { front = rnd(6); back = rnd(8); }
            X.offsets.push_back(X.bases.size() + front);
            X.lengths.push_back(full - front - back);
            X.front.push_back(front);
            X.unclipped.push_back(full);
            for (uint32_t k = 0; k < full; k++) {
                const uint32_t c = rnd(400);
                X.bases.push_back(c == 0 ? 'R' : c == 1 ? 0 : "ACGTacgtNn"[c % 10]);
                X.quals.push_back((char)('!' + rnd(60)));
            }
            std::string id = "pair" + std::to_string(q);
            if (idKind == 1 && e) id += "longer";
            if (idKind == 2) id += " comment";
            if (idKind == 3) id = "";
            if (idKind == 6) id = std::string(longKind ? 254 : 252, 'L');   // 254 bytes after the trim, or before it
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
    A.pieceOffsets = pieceOffsets; A.nPieces = 3;   // no piece names: the BAM rule reads none
    const std::string rg = std::string(rnd(40), 'g');
    std::vector<char> rgBytes(rg.begin(), rg.end());
    auto hRg = exact(rgBytes);   // not NUL-terminated: rgLen bytes are all the rule may read
    A.rg = withRg ? hRg.get() : nullptr;
    A.rgLen = withRg ? (uint32_t)rg.size() : 0;

    const uint64_t recs = 2ull * n;
    const bampairline::Serial none{nullptr};
    std::vector<uint32_t> len(recs);
    std::vector<int32_t> nm(recs);
    uint64_t total = 0;
    int32_t carry = 7;
    for (uint64_t j = 0; j < recs; j++) {
        const bampairline::Fields F = bampairline::fields(A, j, none);
        total += len[j] = bampairline::recordLength(A, F);
        CHECK(F.qlen <= bamline::kMaxQname, "record %llu: QNAME of %u bytes", (unsigned long long)j, F.qlen);
        if (F.nmOwn == bampairline::kNoNm) carried++;
        carry = nm[j] = F.nmOwn == bampairline::kNoNm ? carry : F.nmOwn;
    }
    std::unique_ptr<char[]> block(new char[total + 2 * kGuard]);
    memset(block.get(), 0x7e, total + 2 * kGuard);
    char *out = block.get() + kGuard;
    const bampairline::Serial g{out};
    uint64_t at = 0;
    for (uint64_t j = 0; j < recs; j++) {
        const bampairline::Fields F = bampairline::fields(A, j, g);
        // a fill no record byte sequence relies on: every byte must be stored
        memset(out + at, 0x7e, len[j]);
        bampairline::write(A, j, F, nm[j], at, g);
        const char *r = out + at;
        const uint64_t q = j >> 1;
        const snapgpu_pair_result_t &pr = res[q];
        uint32_t locs[2];
        for (int k = 0; k < 2; k++) locs[k] = pr.status[k] != SNAPGPU_NOT_FOUND ? pr.location[k] : samline::kInvalid;
        const uint32_t first = locs[0] > locs[1], e = (j & 1) == 0 ? first : 1 - first, m = 1 - e;
        CHECK(F.end == e, "record %llu: end", (unsigned long long)j);
        CHECK(get32(r) == len[j] - 4, "record %llu: block_size %u for %u bytes", (unsigned long long)j, get32(r), len[j]);
        CHECK((int32_t)get32(r + 4) == F.refID && (int32_t)get32(r + 8) == F.pos, "record %llu: refID / pos", (unsigned long long)j);
        CHECK((uint8_t)r[12] == F.qlen + 1 && r[36 + F.qlen] == 0, "record %llu: l_read_name", (unsigned long long)j);
        CHECK(get16(r + 16) == F.nCigar && get16(r + 18) == F.flags && get32(r + 20) == F.len, "record %llu: n_cigar / flag / l_seq",
              (unsigned long long)j);
        CHECK((int32_t)get32(r + 24) == F.nextRef && (int32_t)get32(r + 28) == F.nextPos && (int32_t)get32(r + 32) == F.tlen,
              "record %llu: mate fields", (unsigned long long)j);
        const uint32_t fixed = 36 + F.qlen + 1 + 4 * F.nCigar + (F.len + 1) / 2 + F.len;
        CHECK(len[j] == fixed + (withRg ? 4 + A.rgLen : 0) + 15, "record %llu: length", (unsigned long long)j);
        CHECK(memcmp(r + len[j] - 7, "NMi", 3) == 0 && (int32_t)get32(r + len[j] - 4) == nm[j], "record %llu: NM", (unsigned long long)j);
        CHECK(memcmp(r + len[j] - 15, "PGZSNAP", 8) == 0, "record %llu: PG", (unsigned long long)j);
        // the mate rule, restated: flags, the places, who points at whom
        const bool own = locs[e] != samline::kInvalid, mate = locs[m] != samline::kInvalid;
        uint32_t want = 0x1 | ((j & 1) ? 0x80 : 0x40) | (own ? 0 : 0x4) | (mate ? 0 : 0x8) | (own && mate ? 0x2 : 0);
        if (own && pr.direction[e] == SNAPGPU_RC) want |= 0x10;
        if (mate && pr.direction[m] == SNAPGPU_RC) want |= 0x20;
        CHECK(F.flags == want, "record %llu: flags %x, want %x", (unsigned long long)j, F.flags, want);
        if (!own && !mate) CHECK(F.refID == -1 && F.pos == -1 && F.nextRef == -1 && F.nextPos == -1 && F.bin == 4680, "record %llu: unmapped pair", (unsigned long long)j);
        if (!own && mate) CHECK(F.refID == F.nextRef && F.pos == F.nextPos, "record %llu: the unmapped end takes its mate's place", (unsigned long long)j);
        if (own && !mate) CHECK(F.refID == F.nextRef && F.pos == F.nextPos, "record %llu: the mate is unmapped", (unsigned long long)j);
        if (own && locs[e] >= 500) CHECK(F.refID >= 0 && pieceOffsets[F.refID] + (uint32_t)F.pos == locs[e], "record %llu: own place", (unsigned long long)j);
        if (!(own && mate) || F.refID != F.nextRef || F.refID < 0) CHECK(F.tlen == 0, "record %llu: tlen", (unsigned long long)j);
        CHECK(F.nmOwn == (own ? ed[2 * q + e] : bampairline::kNoNm), "record %llu: own NM", (unsigned long long)j);
        CHECK((F.nCigar != 0) == (own && ed[2 * q + e] >= 0 && (F.before || F.after || F.nOps)), "record %llu: CIGAR presence", (unsigned long long)j);
        // getSortInfo
        uint32_t key = samline::kInvalid;
        if (F.refID >= 0 && F.pos >= 0) key = pieceOffsets[F.refID] + (uint32_t)F.pos;
        else if (F.nextRef >= 0 && F.nextPos >= 0) key = pieceOffsets[F.nextRef] + (uint32_t)F.nextPos;
        CHECK(bampairline::sortKey(A, F) == key, "record %llu: sort key", (unsigned long long)j);
        samline::PairFields P;
        bampairline::Fields K;
        bampairline::place(A, j, P, K);
        CHECK(bampairline::sortKey(A, K) == key, "record %llu: sort key from the place alone", (unsigned long long)j);
        at += len[j];
        records++;
    }
    CHECK(at == total, "the records do not fill the buffer");
    for (uint32_t k = 0; k < kGuard; k++)
        CHECK(block[k] == 0x7e && block[kGuard + total + k] == 0x7e, "guard byte %u overwritten", k);
    // no byte keeps the fill by chance alone more often than one in 256: count them
    uint64_t fill = 0;
    for (uint64_t k = 0; k < total; k++) fill += out[k] == 0x7e;
    CHECK(fill * 16 < total + 1024, "%llu of %llu bytes still hold the fill", (unsigned long long)fill, (unsigned long long)total);
}

}  // namespace

int main(int argc, char **argv) {
    const int batches = argc > 1 ? atoi(argv[1]) : 200;
    for (int b = 0; b < batches; b++) oneBatch(1 + rnd(40), b & 1, (b & 2) != 0);
    printf("%d batches, %llu records, %llu carried, %d failed\n", batches, (unsigned long long)records,
           (unsigned long long)carried, failures);
    return failures ? 1 : 0;
}
