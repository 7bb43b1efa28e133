// bgzf_model_test.cpp -- snapgpu_bgzf_compress_model (snap-rnaseq_amd/csrc/host/bgzf.cpp over
// csrc/bgzf_block.h) against zlib's inflater, as a stand-alone program: built from the host sources
// with -fsanitize=address,undefined, so every out-of-range index of the block compressor's arrays
// is an error here.  Every member must carry the BGZF header, inflate alone to exactly its slice of
// the input, end with that slice's CRC32 and length, and take at most m + 31 bytes.
//
//   bgzf_model_test [random cases]
#include <zlib.h>

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

const uint64_t kIn = 0xff00;
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int g_failed = 0;
void fail(const char *what, const char *name, size_t n) {
    if (g_failed++ < 20) printf("FAIL %s: %s (n = %zu)\n", what, name, n);
}

void check(const char *name, const std::vector<unsigned char> &data, int eof) {
    const uint64_t n = data.size();
    uint64_t used = 0;
    std::vector<unsigned char> out(n + (n / kIn + 1) * 31 + 28);
    if (snapgpu_bgzf_compress_model((const char *)data.data(), n, eof, (char *)out.data(), out.size(), &used) != 0)
        return fail("call", name, n);
    uint64_t at = 0, blocks = 0;
    std::vector<unsigned char> back(kIn + 1);
    const uint64_t want = (n + kIn - 1) / kIn;
    for (; blocks < want; blocks++) {
        static const unsigned char hdr[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0};
        const uint64_t m = n - blocks * kIn < kIn ? n - blocks * kIn : kIn;
        if (at + 26 > used || memcmp(out.data() + at, hdr, 16)) return fail("header", name, n);
        const uint64_t size = (uint64_t)out[at + 16] + ((uint64_t)out[at + 17] << 8) + 1;
        if (at + size > used || size > m + 31 || size < 26) return fail("size", name, n);
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) return fail("inflateInit2", name, n);
        z.next_in = out.data() + at + 18;
        z.avail_in = (uInt)(size - 26);
        z.next_out = back.data();
        z.avail_out = (uInt)back.size();
        const int r = inflate(&z, Z_FINISH);
        const bool ok = r == Z_STREAM_END && z.avail_in == 0 && z.total_out == m &&
                        memcmp(back.data(), data.data() + blocks * kIn, m) == 0;
        inflateEnd(&z);
        if (!ok) return fail("inflate", name, n);
        uint32_t crc, isize;
        memcpy(&crc, out.data() + at + size - 8, 4);
        memcpy(&isize, out.data() + at + size - 4, 4);
        if (crc != (uint32_t)crc32(crc32(0L, Z_NULL, 0), data.data() + blocks * kIn, (uInt)m) || isize != m)
            return fail("crc / isize", name, n);
        at += size;
    }
    if (at + (eof ? 28 : 0) != used) return fail("total", name, n);
}

typedef void (*Fill)(std::vector<unsigned char> &);
void zeros(std::vector<unsigned char> &d) { std::fill(d.begin(), d.end(), 0); }
void period2(std::vector<unsigned char> &d) { for (size_t i = 0; i < d.size(); i++) d[i] = (unsigned char)("ab"[i % 2]); }
void period3(std::vector<unsigned char> &d) { for (size_t i = 0; i < d.size(); i++) d[i] = (unsigned char)("xyz"[i % 3]); }
void period259(std::vector<unsigned char> &d) { for (size_t i = 0; i < d.size(); i++) d[i] = (unsigned char)((i % 259) * 7 + (i % 259) / 37); }
void noise(std::vector<unsigned char> &d) { for (auto &b : d) b = (unsigned char)rnd(); }
void bases(std::vector<unsigned char> &d) { for (auto &b : d) b = (unsigned char)("ACGT"[rnd() & 3]); }
void fibonacci(std::vector<unsigned char> &d) {   // byte counts 1, 1, 2, 3, 5, ...: a deep Huffman tree
    size_t at = 0, a = 1, b = 1;
    for (unsigned v = 0; at < d.size(); v++) {
        for (size_t k = 0; k < a && at < d.size(); k++) d[at++] = (unsigned char)v;
        const size_t c = a + b;
        a = b;
        b = c;
    }
    for (size_t i = d.size(); i > 1; i--) std::swap(d[i - 1], d[rnd() % i]);
}

}  // namespace

int main(int argc, char **argv) {
    const int nRandom = argc > 1 ? atoi(argv[1]) : 3000;
    const size_t sizes[] = {0, 1, 2, 3, 4, 257, 258, 259, kIn - 1, kIn, kIn + 1, 3 * kIn + 5};
    const struct { const char *name; Fill f; } fills[] = {{"zeros", zeros}, {"period2", period2}, {"period3", period3},
                                                          {"period259", period259}, {"noise", noise}, {"bases", bases},
                                                          {"fibonacci", fibonacci}};
    int cases = 0;
    for (size_t n : sizes)
        for (const auto &f : fills) {
            std::vector<unsigned char> d(n);
            f.f(d);
            check(f.name, d, cases & 1);
            cases++;
        }
    // a motif at the edge of the window, and across the block boundary, in distinct filler
    for (size_t gap : {(size_t)32768, (size_t)32769, (size_t)(kIn - 20)}) {
        std::vector<unsigned char> d(kIn + 4000);
        for (size_t i = 0; i < d.size(); i++) d[i] = (unsigned char)((i * 2654435761u) >> 13);
        for (size_t i = 0; i < 40; i++) d[gap + i] = d[i] = (unsigned char)rnd();
        check("motif", d, 1);
        cases++;
    }
    // random (size, alphabet, repeat probability): copies of earlier bytes at random distances
    for (int c = 0; c < nRandom; c++) {
        const size_t n = rnd() % 8 == 0 ? rnd() % (2 * kIn + 1) : rnd() % 3000;
        const uint32_t alphabet = 1 + rnd() % 256, repeat = rnd() % 101;
        std::vector<unsigned char> d(n);
        for (size_t i = 0; i < n;) {
            if (i && rnd() % 100 < repeat) {
                const size_t dist = 1 + rnd() % (rnd() % 4 ? (i < 64 ? i : 64) : i), len = 1 + rnd() % 300;
                for (size_t k = 0; k < len && i < n; k++, i++) d[i] = d[i - dist];
            } else {
                d[i++] = (unsigned char)(rnd() % alphabet);
            }
        }
        check("random", d, c & 1);
        cases++;
    }
    printf("bgzf_model: %d cases, %d failed\n", cases, g_failed);
    return g_failed ? 1 : 0;
}
