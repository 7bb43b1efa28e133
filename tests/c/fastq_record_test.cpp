// fastq_record_test.cpp -- the FASTQ record rule (snap-rnaseq_amd/csrc/fastq_record.h), the host
// parser over a buffer (snapgpu_reads_from_fastq_buffer, host/reads.cpp) and snapgpu_reads_clip
// (host/sam.cpp) against a naive byte-at-a-time parser, as a stand-alone program: built from the host
// sources with -fsanitize=address,undefined, every text in a heap block of exactly its size, so a
// read past a line or past the text is an error here.
//
//   fastq_record_test <random texts> [files with one text each ...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fastq_record.h"
#include "snapgpu.h"

namespace snapgpu {   // aligner.hip's pinned allocator, as plain heap memory
void *hostAlloc(size_t bytes, bool *pinned, bool zero) {
    *pinned = false;
    return zero ? calloc(bytes ? bytes : 1, 1) : malloc(bytes ? bytes : 1);
}
void hostFree(void *p, bool) { free(p); }
}  // namespace snapgpu

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int g_failed = 0;
void fail(const char *what, const std::string &name, int clipping) {
    if (g_failed++ < 20) printf("FAIL %s: %s (clipping %d)\n", what, name.c_str(), clipping);
}

struct NaiveRead {
    std::string id, bases, quals;   // quals padded with NUL / cut to the bases
    uint32_t front = 0, len = 0;
};

// One byte at a time, no library call: lines end at '\n' (the last one at the end of the text), are cut
// at their first NUL and lose their trailing CR / LF; four lines make a record.
bool naiveParse(const char *t, uint64_t n, int clipping, std::vector<NaiveRead> &out) {
    std::vector<std::string> lines;
    std::string cur;
    bool open = false;
    for (uint64_t i = 0; i < n; i++) {
        if (t[i] == '\n') { lines.push_back(cur); cur.clear(); open = false; }
        else { cur.push_back(t[i]); open = true; }
    }
    if (open) lines.push_back(cur);
    for (auto &l : lines) {
        size_t z = 0;
        while (z < l.size() && l[z] != 0) z++;
        l.resize(z);
        while (!l.empty() && (l.back() == '\r' || l.back() == '\n')) l.pop_back();
    }
    out.clear();
    for (size_t r = 0; r + 1 <= lines.size() / 4; r++) {
        const std::string &h = lines[4 * r];
        if (h.empty() || h[0] != '@') return false;
        NaiveRead R;
        R.id = h.substr(1);
        R.bases = lines[4 * r + 1];
        R.quals = lines[4 * r + 3];
        R.quals.resize(R.bases.size(), '\0');
        uint32_t len = (uint32_t)R.bases.size(), front = 0;
        if (clipping == 2 || clipping == 3)
            while (len > 0 && R.quals[len - 1] == '#') len--;
        if (clipping == 1 || clipping == 3)
            while (front < len && R.quals[front] == '#') front++;
        if (len - front < 50) { front = 0; len = (uint32_t)R.bases.size(); }
        else len -= front;
        R.front = front;
        R.len = len;
        out.push_back(R);
    }
    return true;
}

void check(const std::string &name, const std::string &text) {
    const uint64_t n = text.size();
    char *t = new char[n ? n : 1];   // exactly the text: the sanitizer sees every byte past it
    if (n) memcpy(t, text.data(), n);
    for (int clipping = 0; clipping <= 3; clipping++) {
        std::vector<NaiveRead> want;
        const bool good = naiveParse(t, n, clipping, want);
        // the header's functions over a newline list of this program's own
        {
            std::vector<uint64_t> nl;
            for (uint64_t i = 0; i < n; i++)
                if (t[i] == '\n') nl.push_back(i);
            if (n && t[n - 1] != '\n') nl.push_back(n);
            const fastqrec::Serial one;
            auto lineStart = [&](uint64_t i) { return i ? nl[i - 1] + 1 : (uint64_t)0; };
            auto lineEnd = [&](uint64_t i) { return nl[i]; };
            bool bad = false;
            for (uint64_t r = 0; r < nl.size() / 4 && !bad; r++) {
                const fastqrec::Record R = fastqrec::record(t, r, lineStart, lineEnd, one);
                if (R.bad) { bad = true; break; }
                if (r >= want.size()) { fail("header: a record the naive parser does not have", name, clipping); break; }
                const NaiveRead &W = want[r];
                if (std::string(t + R.idAt, R.idLen) != W.id || std::string(t + R.baseAt, R.baseLen) != W.bases)
                    fail("header: id or bases", name, clipping);
                const char *q = t + R.qualAt;
                const uint32_t nq = R.qualLen;
                uint32_t front = 7, len = 7;
                fastqrec::clip([=](uint64_t k) { return k < nq ? q[k] : (char)0; }, R.baseLen, clipping, front, len, one);
                if (front != W.front || len != W.len) fail("header: clip", name, clipping);
            }
            if (bad == good) fail("header: bad-header flag", name, clipping);
        }
        // the buffer parser and snapgpu_reads_clip
        snapgpu_reads_t *rd = snapgpu_reads_from_fastq_buffer(n ? t : nullptr, n, "case");
        if (!good) {
            if (rd || strcmp(snapgpu_last_error(), "FASTQ record without '@' header in case")) fail("parser: error expected", name, clipping);
            if (rd) snapgpu_reads_free(rd);
            continue;
        }
        if (!rd) { fail("parser: refused", name, clipping); continue; }
        if (clipping && snapgpu_reads_clip(rd, clipping, nullptr, nullptr) != SNAPGPU_OK) fail("clip: refused", name, clipping);
        if (rd->n != want.size()) fail("parser: n", name, clipping);
        else {
            uint64_t o = 0, io = 0;
            for (uint64_t r = 0; r < rd->n; r++) {
                const NaiveRead &W = want[r];
                const uint32_t full = (uint32_t)W.bases.size();
                if (rd->offsets[r] != o + W.front || rd->lengths[r] != W.len) fail("parser: clipped extent", name, clipping);
                if (memcmp(rd->bases + o, W.bases.data(), full) || memcmp(rd->quals + o, W.quals.data(), full))
                    fail("parser: bases or qualities", name, clipping);
                if (rd->idOffsets[r] != io || rd->idLengths[r] != W.id.size() || memcmp(rd->ids + io, W.id.data(), W.id.size()))
                    fail("parser: id", name, clipping);
                if (clipping && (rd->frontClipped[r] != W.front || rd->unclippedLength[r] != full))
                    fail("clip: state", name, clipping);
                o += full;
                io += W.id.size();
            }
            if (rd->totalBytes != o) fail("parser: totalBytes", name, clipping);
            for (int k = 0; k < 64; k++)
                if (rd->bases[o + k] || rd->quals[o + k]) { fail("parser: slack", name, clipping); break; }
        }
        snapgpu_reads_free(rd);
    }
    delete[] t;
}

std::string randomText() {
    static const char *eols[] = {"\n", "\n", "\n", "\r\n", "\r\r\n"};
    static const char alphabet[] = {'A', 'C', 'G', 'T', 'N', '#', '#', 'I', '@', '+', ' ', '\r', '\0', '\n'};
    std::string t;
    const uint32_t recs = rnd() % 9;
    for (uint32_t r = 0; r < recs; r++) {
        const char *eol = eols[rnd() % 5];
        if (rnd() % 16 == 0) {   // four lines of anything
            for (int l = 0; l < 4; l++) {
                for (uint32_t k = rnd() % 40; k; k--) t.push_back(alphabet[rnd() % sizeof alphabet]);
                t += eol;
            }
            continue;
        }
        const uint32_t n = rnd() % 4 == 0 ? 45 + rnd() % 12 : rnd() % 130;
        t.push_back(rnd() % 64 ? '@' : 'x');
        for (uint32_t k = rnd() % 30; k; k--) t.push_back(alphabet[rnd() % 12]);
        t += eol;
        for (uint32_t k = 0; k < n; k++) t.push_back(rnd() % 97 ? "ACGTN"[rnd() % 5] : '\0');
        t += eol;
        t += rnd() % 4 ? "+" : "@+x";
        t += eol;
        const uint32_t f = rnd() % 3 ? rnd() % 8 : rnd() % (n + 1), b = rnd() % 3 ? rnd() % 8 : rnd() % (n + 1);
        const uint32_t nq = rnd() % 8 ? n : rnd() % (n + 9);
        for (uint32_t k = 0; k < nq; k++) t.push_back(k < f || k + b >= n ? '#' : (rnd() % 50 ? 'I' : '#'));
        t += eol;
    }
    switch (rnd() % 5) {
        case 0: t += "@t"; break;
        case 1: t += "@t\nAC\n"; break;
        case 2: t += "@t\nAC\n+\n"; break;
        case 3: while (!t.empty() && (t.back() == '\n' || t.back() == '\r')) t.pop_back(); break;
        default: break;
    }
    return t;
}

}  // namespace

int main(int argc, char **argv) {
    const int nRandom = argc > 1 ? atoi(argv[1]) : 3000;
    int cases = 0;
    for (int k = 2; k < argc; k++) {
        FILE *f = fopen(argv[k], "rb");
        if (!f) { printf("cannot open %s\n", argv[k]); return 2; }
        std::string text;
        char buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
        fclose(f);
        check(argv[k], text);
        cases++;
    }
    for (int k = 0; k < nRandom; k++) {
        check("random " + std::to_string(k), randomText());
        cases++;
    }
    printf("%d cases, %d failed\n", cases, g_failed);
    return g_failed ? 1 : 0;
}
