// inflate_model_test.cpp -- snapgpu_bgzf_inflate_model (snap-rnaseq_amd/csrc/host/inflate.cpp over
// csrc/inflate_block.h, the decoder the device kernel compiles) against zlib, as a stand-alone
// program: built from the host sources with -fsanitize=address,undefined, every buffer exactly as
// long as its contents, so a read outside a member or a write outside its output is an error here.
//
// Seeded random inputs are compressed by zlib at mixed levels, strategies and memLevels into BGZF
// members of mixed sizes, and by snapgpu_bgzf_compress_model; the model must give the input back.
// Each stream is then damaged -- bytes flipped inside a member's deflate bytes, the deflate bytes
// cut short with BSIZE adjusted, the trailer edited -- and the model must do what zlib does with
// the damaged member: refuse it, or accept it with the same bytes.
//
//   inflate_model_test [random cases]
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

typedef std::vector<unsigned char> Bytes;

const uint64_t kIn = 0xff00;
uint64_t g_state = 0x2545f4914f6cdd1dull;
uint32_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int g_failed = 0, g_accepted = 0, g_refused = 0;
void fail(const char *what, int c) {
    if (g_failed++ < 20) printf("FAIL %s (case %d)\n", what, c);
}

struct Member { size_t at, size, def, defLen; };   // in the stream: start, size, deflate bytes

void put16(Bytes &b, uint32_t v) { b.push_back((unsigned char)v); b.push_back((unsigned char)(v >> 8)); }
void put32(Bytes &b, uint32_t v) { put16(b, v & 0xffffu); put16(b, v >> 16); }

// one member around raw deflate bytes
void appendMember(Bytes &s, std::vector<Member> &mem, const unsigned char *def, size_t defLen, uint32_t crc, uint32_t isize) {
    static const unsigned char hdr[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0};
    const size_t at = s.size(), size = 18 + defLen + 8;
    s.insert(s.end(), hdr, hdr + 16);
    put16(s, (uint32_t)(size - 1));
    s.insert(s.end(), def, def + defLen);
    put32(s, crc);
    put32(s, isize);
    mem.push_back(Member{at, size, at + 18, defLen});
}

// zlib's members of d: blocks of `block` bytes, each with its own level, strategy and memLevel
bool zlibStream(const Bytes &d, size_t block, Bytes &s, std::vector<Member> &mem) {
    static const int strategies[5] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
    Bytes def(block + block / 8 + 1024);
    for (size_t k = 0; k < d.size(); k += block) {
        const size_t m = d.size() - k < block ? d.size() - k : block;
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, (int)(rnd() % 10), Z_DEFLATED, -15, 1 + (int)(rnd() % 9), strategies[rnd() % 5]) != Z_OK) return false;
        z.next_in = const_cast<unsigned char *>(d.data() + k);
        z.avail_in = (uInt)m;
        z.next_out = def.data();
        z.avail_out = (uInt)def.size();
        const int r = deflate(&z, Z_FINISH);
        const size_t len = z.total_out;
        deflateEnd(&z);
        if (r != Z_STREAM_END || 18 + len + 8 > 65536) return false;
        appendMember(s, mem, def.data(), len, (uint32_t)crc32(crc32(0L, Z_NULL, 0), d.data() + k, (uInt)m), (uint32_t)m);
    }
    return true;
}

std::vector<Member> membersOf(const Bytes &s) {   // of a stream with the 18-byte header
    std::vector<Member> mem;
    for (size_t at = 0; at + 26 <= s.size();) {
        const size_t size = (size_t)s[at + 16] + ((size_t)s[at + 17] << 8) + 1;
        mem.push_back(Member{at, size, at + 18, size - 26});
        at += size;
    }
    return mem;
}

// the model over a stream held in a buffer of exactly its size -> its return code; out: exactly the bytes
int model(const Bytes &stream, Bytes &out) {
    Bytes exact(stream);   // a fresh allocation of stream.size() bytes
    uint64_t used = 0;
    int rc = snapgpu_bgzf_inflate_model((const char *)exact.data(), exact.size(), nullptr, 0, &used);
    if (rc != 0 && used == 0) return rc;   // the walk refused it (or nothing to write)
    out.assign(used, 0);
    rc = snapgpu_bgzf_inflate_model((const char *)exact.data(), exact.size(), (char *)out.data(), out.size(), &used);
    return rc;
}

// zlib's verdict on one member of s: accepted (eof at the last byte, ISIZE bytes, the trailer's CRC32) and its bytes
bool zlibMember(const Bytes &s, const Member &M, Bytes &out) {
    Bytes def(s.begin() + M.def, s.begin() + M.def + M.defLen);
    uint32_t crc, isize;
    memcpy(&crc, s.data() + M.at + M.size - 8, 4);
    memcpy(&isize, s.data() + M.at + M.size - 4, 4);
    Bytes back(65536 + 1);
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    unsigned char none = 0;
    z.next_in = def.empty() ? &none : def.data();
    z.avail_in = (uInt)def.size();
    z.next_out = back.data();
    z.avail_out = (uInt)back.size();
    const int r = inflate(&z, Z_FINISH);
    const bool ok = r == Z_STREAM_END && z.avail_in == 0 && z.total_out == isize &&
                    crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), back.data(), (uInt)z.total_out);
    out.assign(back.begin(), back.begin() + z.total_out);
    inflateEnd(&z);
    return ok;
}

// A damaged stream: the model must agree with zlib about the damaged member k (the others are intact).
void checkDamaged(const Bytes &s, const std::vector<Member> &mem, size_t k, const Bytes &data, const std::vector<size_t> &outAt,
                  const char *what, int c) {
    Bytes out, want;
    uint32_t isize;
    memcpy(&isize, s.data() + mem[k].at + mem[k].size - 4, 4);
    const bool zok = isize <= 65536 && zlibMember(s, mem[k], want);
    const int rc = model(s, out);
    if (!zok) {
        g_refused++;
        if (rc != SNAPGPU_EFORMAT) fail(what, c);
        return;
    }
    g_accepted++;
    // zlib accepts: so must the model, with the other members' bytes around zlib's for this one
    Bytes all(data.begin(), data.begin() + outAt[k]);
    all.insert(all.end(), want.begin(), want.end());
    all.insert(all.end(), data.begin() + outAt[k + 1], data.end());
    if (rc != 0 || out != all) fail(what, c);
}

void damage(const Bytes &s, const std::vector<Member> &mem, const Bytes &data, int c) {
    if (mem.empty()) return;
    std::vector<size_t> outAt(mem.size() + 1, 0);
    for (size_t k = 0; k < mem.size(); k++) {
        uint32_t isize;
        memcpy(&isize, s.data() + mem[k].at + mem[k].size - 4, 4);
        outAt[k + 1] = outAt[k] + isize;
    }
    const size_t k = rnd() % mem.size();
    const Member &M = mem[k];
    if (M.defLen) {   // flips inside the deflate bytes
        Bytes t(s);
        for (uint32_t f = 1 + rnd() % 3; f > 0; f--) t[M.def + rnd() % M.defLen] ^= (unsigned char)(1u << (rnd() % 8));
        checkDamaged(t, mem, k, data, outAt, "flip", c);
    }
    {   // the deflate bytes cut short, BSIZE adjusted
        const size_t keep = M.defLen ? rnd() % M.defLen : 0, cut = M.defLen - keep;
        Bytes t(s.begin(), s.begin() + M.def + keep);
        t.insert(t.end(), s.begin() + M.def + M.defLen, s.end());
        const size_t size = M.size - cut;
        t[M.at + 16] = (unsigned char)(size - 1);
        t[M.at + 17] = (unsigned char)((size - 1) >> 8);
        std::vector<Member> m2(mem);
        m2[k].size = size;
        m2[k].defLen = keep;
        for (size_t j = k + 1; j < m2.size(); j++) { m2[j].at -= cut; m2[j].def -= cut; }
        checkDamaged(t, m2, k, data, outAt, "truncate", c);
    }
    {   // one trailer byte: the CRC32 or ISIZE
        Bytes t(s);
        t[M.at + M.size - 8 + rnd() % 8] ^= (unsigned char)(1u << (rnd() % 8));
        checkDamaged(t, mem, k, data, outAt, "trailer", c);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const int nRandom = argc > 1 ? atoi(argv[1]) : 3000;
    for (int c = 0; c < nRandom; c++) {
        // random (size, alphabet, repeat probability): copies of earlier bytes at random distances
        const size_t n = rnd() % 8 == 0 ? rnd() % (2 * kIn + 1) : rnd() % 3000;
        const uint32_t alphabet = 1 + rnd() % 256, repeat = rnd() % 101;
        Bytes d(n);
        for (size_t i = 0; i < n;) {
            if (i && rnd() % 100 < repeat) {
                const size_t dist = 1 + rnd() % (rnd() % 4 ? (i < 64 ? i : 64) : i), len = 1 + rnd() % 300;
                for (size_t k = 0; k < len && i < n; k++, i++) d[i] = d[i - dist];
            } else {
                d[i++] = (unsigned char)(rnd() % alphabet);
            }
        }
        Bytes s, out;
        std::vector<Member> mem;
        const size_t block = rnd() % 4 == 0 ? 1 + rnd() % 2000 : kIn;
        if (!zlibStream(d, block, s, mem)) { fail("zlib could not compress", c); continue; }
        if (rnd() % 4 == 0) appendMember(s, mem, (const unsigned char *)"\3\0", 2, 0, 0);   // the EOF block
        if (model(s, out) != 0 || out != d) fail("zlib's stream", c);
        damage(s, mem, d, c);
        // the device compressor's stream of the same bytes
        Bytes own(n + (n / kIn + 1) * 31 + 28);
        uint64_t used = 0;
        if (snapgpu_bgzf_compress_model((const char *)d.data(), n, c & 1, (char *)own.data(), own.size(), &used) != 0) {
            fail("compress_model", c);
            continue;
        }
        own.resize(used);
        if (model(own, out) != 0 || out != d) fail("the compressor model's stream", c);
        damage(own, membersOf(own), d, c);
    }
    printf("inflate_model: %d cases, %d damaged members accepted as zlib does, %d refused as zlib does, %d failed\n", nRandom,
           g_accepted, g_refused, g_failed);
    return g_failed ? 1 : 0;
}
