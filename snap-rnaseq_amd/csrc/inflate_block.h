// inflate_block.h -- the raw deflate stream (RFC 1951) of one BGZF member, inflated into a window
// of at most 65,536 bytes; specified once for host and device.  bgzf_block.h's counterpart.
//
// The host model (host/inflate.cpp, one thread per member) and the device kernel (inflate.hip, one
// 64-lane wave per member) both call inflateMember() below, so every decision -- what a code set
// is, which symbol the next bits are, which input is refused and with which status -- is stated
// here.  As in fastq_record.h the rule is a template over a "group" G, the lanes that share one
// member.  Every member of a group calls with the same arguments and receives the same results;
// the stream position, the bit buffer and the output position are the same in all of them.
//
//   g.forEach(n, fn)            fn(k) for every k < n, each k by one member of the group
//   g.serial(fn)                fn() by one member; its uint32_t result to all
//   g.uni(x)                    x, which all members hold alike, marked as such
//   g.sync()                    what members wrote to the Work before is read by all after
//   g.load64(p)                 the 8 bytes at p, little-endian (p unaligned)
//   g.xorAll(v)                 xor of the members' v
//   g.copyIn(win, pos, src, n)  win[pos + k] = src[k], k < n
//   g.copyMatch(win, pos, d, n) win[pos + k] = win[pos - d + matchSource(k, d)], k < n
//   g.store(win, pos, b)        win[pos] = b
// Serial (below) is one host thread; inflate.hip has the wave.
//
// Input: the member's deflate bytes def[0 .. n) followed by its 8 trailer bytes; nothing outside
// def[0 .. n + 8) is read.  Output: bytes [0, isize) of the Work's window, isize <= kMaxOut; nothing
// else of the window is written.  The caller moves the window to the member's place.
//
// A stream is accepted exactly when zlib's raw inflater accepts it with eof at its last byte, isize
// bytes out and their CRC32 equal to the trailer's (inflate.c / inftrees.c are the reading of
// RFC 1951 followed where it leaves a choice: an incomplete literal/length or distance set is
// accepted only as a single code of one bit, a distance set may be empty, HLIT <= 286 and
// HDIST <= 30).
//
// Codes: a set's symbols sorted by (length, symbol) with the count of each length is the canonical
// code (RFC 1951 3.2.2); slowDecode() walks it one bit at a time, and the table of the first
// kFast bits is slowDecode() of every index, which is what makes it a loop over independent
// entries.  Codes longer than the table take slowDecode() again.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bgzf_block.h"

#if defined(__HIPCC__)
#define INF_HD __host__ __device__ inline
#else
#define INF_HD inline
#endif

namespace inflateblock {

constexpr uint32_t kMaxOut = 65536;       // the largest ISIZE of a BGZF member
constexpr uint32_t kLitFast = 10, kDistFast = 8, kClFast = 7;
constexpr uint32_t kLit = 288, kDist = 32, kCl = 19, kEob = 256;
constexpr uint32_t kMaxLit = 286, kMaxDist = 30;   // symbols a stream may declare and use

enum Status : uint32_t {
    kOk = 0,
    kBlockType = 1,          // BTYPE 3
    kStoredLength = 2,       // LEN != ~NLEN
    kTooManySymbols = 3,     // HLIT > 286 or HDIST > 30
    kCodeLengthSet = 4,      // the code-length set is over-subscribed or incomplete
    kRepeat = 5,             // symbol 16 with no length before it, or a run past HLIT + HDIST
    kNoEndOfBlock = 6,       // symbol 256 has no code
    kLitOversubscribed = 7,
    kLitIncomplete = 8,
    kDistOversubscribed = 9,
    kDistIncomplete = 10,
    kNoCode = 11,            // bits that are no code of an incomplete (or empty) set
    kLengthSymbol = 12,      // literal/length symbol 286 or 287
    kDistanceSymbol = 13,    // distance symbol 30 or 31
    kDistanceTooFar = 14,    // a distance that reaches before the member's first byte
    kOutputOverflow = 15,    // output that would pass ISIZE
    kInputExhausted = 16,    // the stream needs bits after its last byte
    kTrailingBytes = 17,     // whole bytes left after the final block
    kSizeMismatch = 18,      // fewer bytes out than ISIZE
    kCrcMismatch = 19,
    kStatusCount = 20
};

#if !defined(__HIP_DEVICE_COMPILE__)
inline const char *statusName(uint32_t s) {
    static const char *const names[kStatusCount] = {
        "ok", "block type 3", "stored block with LEN != ~NLEN", "more than 286 literal/length or 30 distance codes",
        "bad code-length set", "bad code-length repeat", "no end-of-block code", "over-subscribed literal/length set",
        "incomplete literal/length set", "over-subscribed distance set", "incomplete distance set",
        "bits that are no code", "literal/length symbol 286 or 287", "distance symbol 30 or 31",
        "distance before the member's first byte", "output longer than ISIZE", "deflate stream ends early",
        "bytes left after the final block", "output shorter than ISIZE", "CRC32 mismatch"};
    return s < kStatusCount ? names[s] : "unknown status";
}
#endif

// One member of a BGZF stream as the member walk (host/inflate.cpp) found it.
struct Member {
    uint64_t inStart;    // its first byte in the stream
    uint64_t outStart;   // where its output goes
    uint32_t inSize;     // BSIZE + 1
    uint32_t outSize;    // ISIZE
    uint32_t defOff;     // its deflate bytes begin here: 12 + XLEN
    uint32_t pad;
};

// A canonical code of at most N symbols with a table of its first FAST bits.
template <uint32_t N, uint32_t FAST>
struct Code {
    uint16_t fast[1u << FAST];   // symbol << 4 | length of the code that index's low bits begin with; 0: none that short
    uint16_t sym[N];             // the used symbols by (length, symbol)
    uint16_t count[16];          // codes of each length
    uint16_t offs[16];           // scratch of setupCode
};

struct Work {
    uint32_t win[kMaxOut / 4 + 16];   // the member's output; the words after it are never written
    Code<kLit, kLitFast> lit;
    Code<kDist, kDistFast> dist;
    Code<kCl, kClFast> cl;
    uint8_t lens[kLit + kDist];       // the code lengths a block header declares
    uint32_t crcTab[256], xpow[16];   // bgzf_block.h's crcTableEntry / crcXpow
};

struct Serial {
    template <class F>
    void forEach(uint32_t n, F fn) const {
        for (uint32_t k = 0; k < n; k++) fn(k);
    }
    template <class F>
    uint32_t serial(F fn) const { return fn(); }
    uint32_t uni(uint32_t x) const { return x; }
    void sync() const {}
    uint64_t load64(const uint8_t *p) const {
        uint64_t v;
        memcpy(&v, p, 8);
        return v;
    }
    uint32_t xorAll(uint32_t v) const { return v; }
    void copyIn(uint8_t *win, uint32_t pos, const uint8_t *src, uint32_t n) const { memcpy(win + pos, src, n); }
    inline void copyMatch(uint8_t *win, uint32_t pos, uint32_t dist, uint32_t n) const;
    void store(uint8_t *win, uint32_t pos, uint32_t b) const { win[pos] = (uint8_t)b; }
};

// Byte k of a match of distance d is byte matchSource(k, d) of the d bytes before the match: what
// copying byte by byte gives, without reading a byte of the match itself.
INF_HD uint32_t matchSource(uint32_t k, uint32_t d) { return k < d ? k : k % d; }

inline void Serial::copyMatch(uint8_t *win, uint32_t pos, uint32_t dist, uint32_t n) const {
    for (uint32_t k = 0; k < n; k++) win[pos + k] = win[pos - dist + matchSource(k, dist)];
}

// ---------------------------------------------------------------- codes
// The code that `bits` (first bit lowest) begins with, among the codes of at most maxLen bits.
template <class C>
INF_HD bool slowDecode(const C &c, uint32_t bits, uint32_t maxLen, uint32_t &sym, uint32_t &len) {
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= maxLen; l++) {
        code |= bits & 1u;
        bits >>= 1;
        const uint32_t count = c.count[l];
        if (code < first + count) {
            sym = c.sym[index + (code - first)];
            len = l;
            return true;
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return false;
}

// One member of the group: counts, Kraft sum and sorted symbols of the n code lengths.
// -> 0: complete (or no code at all), 1: over-subscribed, 2: incomplete, 3: one code of one bit
template <class C>
INF_HD uint32_t setupCode(C &c, const uint8_t *lens, uint32_t n) {
    for (uint32_t b = 0; b < 16; b++) c.count[b] = 0;
    for (uint32_t i = 0; i < n; i++) c.count[lens[i] & 15u]++;
    const uint32_t unused = c.count[0];
    c.count[0] = 0;
    int32_t left = 1;
    uint32_t maxLen = 0;
    for (uint32_t b = 1; b < 16; b++) {
        left = left * 2 - (int32_t)c.count[b];
        if (left < 0) return 1;
        if (c.count[b]) maxLen = b;
    }
    c.offs[1] = 0;
    for (uint32_t b = 1; b < 15; b++) c.offs[b + 1] = (uint16_t)(c.offs[b] + c.count[b]);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = lens[i] & 15u;
        if (l) c.sym[c.offs[l]++] = (uint16_t)i;
    }
    if (unused == n || left == 0) return 0;
    return maxLen == 1 ? 3 : 2;
}

template <class C, class G>
INF_HD void fillFast(C &c, uint32_t fastBits, const G &g) {
    g.forEach(1u << fastBits, [&c, fastBits](uint32_t i) {
        uint32_t sym = 0, len = 0;
        c.fast[i] = slowDecode(c, i, fastBits, sym, len) ? (uint16_t)(sym << 4 | len) : (uint16_t)0;
    });
}

// setupCode and fillFast -> setupCode's result
template <class C, class G>
INF_HD uint32_t buildCode(C &c, uint32_t fastBits, const uint8_t *lens, uint32_t n, const G &g) {
    g.sync();
    const uint32_t r = g.serial([&c, lens, n]() { return setupCode(c, lens, n); });
    if (r == 1 || r == 2) return r;
    fillFast(c, fastBits, g);
    g.sync();
    return r;
}

// ---------------------------------------------------------------- bits
// The stream from bit 8 * ip - cnt on: buf's low cnt bits are its next bits.
struct Bits {
    const uint8_t *in;
    uint32_t n;     // deflate bytes; in[n .. n + 8) is the member's trailer
    uint64_t buf;
    uint32_t cnt;
    uint32_t ip;    // bytes taken into buf
};

// cnt >= 56 after it.  Past the deflate bytes the stream goes on with the trailer's bytes and then
// zeros; exhausted() tells.
template <class G>
INF_HD void refill(Bits &b, const G &g) {
    const uint64_t v = b.ip <= b.n ? g.load64(b.in + b.ip) : 0ull;
    b.buf |= v << b.cnt;
    b.ip += (63u - b.cnt) >> 3;
    b.cnt |= 56u;
}

template <class G>
INF_HD void need(Bits &b, uint32_t bits, const G &g) {
    if (b.cnt < bits) refill(b, g);
}

INF_HD uint32_t take(Bits &b, uint32_t bits) {
    const uint32_t v = (uint32_t)b.buf & ((1u << bits) - 1u);
    b.buf >>= bits;
    b.cnt -= bits;
    return v;
}

// bits were taken that the stream does not have
INF_HD bool exhausted(const Bits &b) { return 8u * b.ip - b.cnt > 8u * b.n; }

// The next symbol of code c, taken from the stream; false: the bits are no code.
template <class C, class G>
INF_HD bool nextSymbol(const C &c, uint32_t fastBits, Bits &b, uint32_t &sym, const G &g) {
    const uint32_t e = g.uni(c.fast[(uint32_t)b.buf & ((1u << fastBits) - 1u)]);
    uint32_t len;
    if (e) {
        sym = e >> 4;
        len = e & 15u;
    } else {
        uint32_t s = 0, l = 0;
        const bool found = slowDecode(c, (uint32_t)b.buf, 15, s, l);
        if (!g.uni(found)) return false;
        sym = g.uni(s);
        len = g.uni(l);
    }
    b.buf >>= len;
    b.cnt -= len;
    return true;
}

// RFC 1951 3.2.5
INF_HD void lengthOf(uint32_t sym, uint32_t &base, uint32_t &extra) {
    const uint32_t s = sym - 257u;
    if (s < 8u) { base = 3u + s; extra = 0; return; }
    if (s == 28u) { base = 258; extra = 0; return; }
    extra = (s >> 2) - 1u;
    base = 3u + ((4u + (s & 3u)) << extra);
}

INF_HD void distanceOf(uint32_t sym, uint32_t &base, uint32_t &extra) {
    if (sym < 4u) { base = 1u + sym; extra = 0; return; }
    extra = (sym >> 1) - 1u;
    base = 1u + ((2u + (sym & 1u)) << extra);
}

// ---------------------------------------------------------------- blocks
// BTYPE 1: the fixed code lengths (RFC 1951 3.2.6) through the same construction.
template <class G>
INF_HD void fixedCodes(Work &W, const G &g) {
    uint8_t *lens = W.lens;
    g.forEach(kLit + kDist, [lens](uint32_t i) {
        lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < kLit ? 8u : 5u);
    });
    buildCode(W.lit, kLitFast, W.lens, kLit, g);
    buildCode(W.dist, kDistFast, W.lens + kLit, kDist, g);
}

// BTYPE 2: the block's header into W.lit and W.dist
template <class G>
INF_HD uint32_t dynamicCodes(Work &W, Bits &b, const G &g) {
    const uint8_t order[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    need(b, 14, g);
    const uint32_t nLit = take(b, 5) + 257u, nDist = take(b, 5) + 1u, nCl = take(b, 4) + 4u;
    if (exhausted(b)) return kInputExhausted;
    if (nLit > kMaxLit || nDist > kMaxDist) return kTooManySymbols;
    for (uint32_t i = 0; i < kCl; i++) {
        uint32_t l = 0;
        if (i < nCl) {
            need(b, 3, g);
            l = take(b, 3);
        }
        W.lens[order[i]] = (uint8_t)l;
    }
    if (exhausted(b)) return kInputExhausted;
    if (buildCode(W.cl, kClFast, W.lens, kCl, g) != 0) return kCodeLengthSet;
    const uint32_t total = nLit + nDist;
    uint32_t i = 0, prev = 0;
    while (i < total) {
        need(b, 7 + 7, g);
        uint32_t sym;
        if (!nextSymbol(W.cl, kClFast, b, sym, g)) return exhausted(b) ? kInputExhausted : kNoCode;
        if (sym < 16u) {
            if (exhausted(b)) return kInputExhausted;
            W.lens[i++] = (uint8_t)sym;
            prev = sym;
            continue;
        }
        uint32_t rep, val = 0;
        if (sym == 16u) {
            rep = 3u + take(b, 2);
            val = prev;
        } else if (sym == 17u) {
            rep = 3u + take(b, 3);
        } else {
            rep = 11u + take(b, 7);
        }
        if (exhausted(b)) return kInputExhausted;
        if ((sym == 16u && i == 0) || i + rep > total) return kRepeat;
        for (uint32_t k = 0; k < rep; k++) W.lens[i++] = (uint8_t)val;
        prev = val;
    }
    g.sync();
    if (g.uni(W.lens[kEob]) == 0) return kNoEndOfBlock;
    uint32_t r = buildCode(W.lit, kLitFast, W.lens, nLit, g);
    if (r == 1) return kLitOversubscribed;
    if (r == 2) return kLitIncomplete;
    r = buildCode(W.dist, kDistFast, W.lens + nLit, nDist, g);
    if (r == 1) return kDistOversubscribed;
    if (r == 2) return kDistIncomplete;
    return kOk;
}

// The symbols of a block coded with W.lit and W.dist, up to its end-of-block.
template <class G>
INF_HD uint32_t codedBlock(Work &W, Bits &b, uint32_t &pos, uint32_t isize, const G &g) {
    uint8_t *win = reinterpret_cast<uint8_t *>(W.win);
    for (;;) {
        need(b, 15 + 5, g);
        uint32_t sym;
        if (!nextSymbol(W.lit, kLitFast, b, sym, g)) return exhausted(b) ? kInputExhausted : kNoCode;
        if (sym < kEob) {
            if (exhausted(b)) return kInputExhausted;
            if (pos >= isize) return kOutputOverflow;
            g.store(win, pos, sym);
            pos++;
            continue;
        }
        if (sym == kEob) return exhausted(b) ? kInputExhausted : kOk;
        if (sym >= kMaxLit) return exhausted(b) ? kInputExhausted : kLengthSymbol;
        uint32_t base, extra;
        lengthOf(sym, base, extra);
        const uint32_t len = base + take(b, extra);
        need(b, 15 + 13, g);
        if (!nextSymbol(W.dist, kDistFast, b, sym, g)) return exhausted(b) ? kInputExhausted : kNoCode;
        if (sym >= kMaxDist) return exhausted(b) ? kInputExhausted : kDistanceSymbol;
        distanceOf(sym, base, extra);
        const uint32_t dist = base + take(b, extra);
        if (exhausted(b)) return kInputExhausted;
        if (dist > pos) return kDistanceTooFar;
        if (len > isize - pos) return kOutputOverflow;
        g.copyMatch(win, pos, dist, len);
        pos += len;
    }
}

// BTYPE 0
template <class G>
INF_HD uint32_t storedBlock(Work &W, Bits &b, uint32_t &pos, uint32_t isize, const G &g) {
    take(b, b.cnt & 7u);   // to the next byte of the stream
    need(b, 32, g);
    const uint32_t len = take(b, 16), nlen = take(b, 16);
    if (exhausted(b)) return kInputExhausted;
    if (len != (~nlen & 0xffffu)) return kStoredLength;
    const uint32_t at = b.ip - b.cnt / 8u;
    if (len > b.n - at) return kInputExhausted;
    if (len > isize - pos) return kOutputOverflow;
    g.copyIn(reinterpret_cast<uint8_t *>(W.win), pos, b.in + at, len);
    pos += len;
    b.ip = at + len;
    b.buf = 0;
    b.cnt = 0;
    return kOk;
}

// the CRC32 of the window's first size bytes: bgzf_block.h's slices, each brought to the end
template <class G>
INF_HD uint32_t windowCrc(const Work &W, uint32_t size, const G &g) {
    uint32_t part = 0;
    const uint32_t slices = (size + bgzfblock::kCrcSlice - 1) / bgzfblock::kCrcSlice;
    g.forEach(slices, [&W, &part, size](uint32_t s) {
        const uint32_t p = s * bgzfblock::kCrcSlice, len = size - p < bgzfblock::kCrcSlice ? size - p : bgzfblock::kCrcSlice;
        part ^= bgzfblock::crcAdvance(bgzfblock::crcSlice(W.crcTab, W.win, p, len), size - p - len, W.xpow);
    });
    return g.xorAll(part);
}

// The member's deflate bytes def[0 .. n) into W.win[0 .. isize) -> Status.  W.crcTab and W.xpow
// are set by the caller.
template <class G>
INF_HD uint32_t inflateMember(const uint8_t *def, uint32_t n, uint32_t isize, uint32_t crcWant, Work &W, const G &g) {
    if (isize > kMaxOut) return kOutputOverflow;
    Bits b{def, n, 0, 0, 0};
    uint32_t pos = 0;
    for (;;) {
        need(b, 3, g);
        const uint32_t final = take(b, 1), type = take(b, 2);
        if (exhausted(b)) return kInputExhausted;
        uint32_t st = kOk;
        if (type == 0u) {
            st = storedBlock(W, b, pos, isize, g);
        } else if (type == 3u) {
            st = kBlockType;
        } else {
            if (type == 1u) fixedCodes(W, g);
            else st = dynamicCodes(W, b, g);
            if (st == kOk) st = codedBlock(W, b, pos, isize, g);
        }
        if (st != kOk) return st;
        if (final) break;
    }
    if (8u * b.n - (8u * b.ip - b.cnt) >= 8u) return kTrailingBytes;
    if (pos != isize) return kSizeMismatch;
    g.sync();
    if (windowCrc(W, isize, g) != crcWant) return kCrcMismatch;
    return kOk;
}

}  // namespace inflateblock
