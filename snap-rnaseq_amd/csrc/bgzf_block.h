// bgzf_block.h -- one BGZF member (a gzip member with the BC extra field around one raw deflate
// stream) of a block of m <= 0xff00 input bytes, specified once for host and device.
//
// The member is a pure function of the block's bytes.  The device compressor (bgzf.hip, one
// workgroup per block) and the host model (host/bgzf.cpp, one serial loop per block) both follow
// the steps below and call the same functions of this header for every decision, so their bytes
// are equal; nothing depends on the order in which lanes run (the shared updates are max, add, xor
// and or of integers).
//
//   data    the block in 32-bit words, zero bytes after byte m (load32 reads whole words)
//   find    positions are taken in windows of kWindow: every position p of a window with 4 bytes
//           left reads table[hash4(load32(p))] -- the largest position before the window with that
//           hash --, then every such p stores max(table[h], p + 1).  bestMatch() extends that
//           candidate and the distances 1 .. 4 (the window hides nearer positions from the table;
//           runs of one byte and short periods live there) and keeps the longest, the first on ties
//   parse   greedy from byte 0: at p a match of bestMatch's length if it found one, else a literal;
//           next = p + max(1, len).  The device marks the parse by pointer jumping over chunks of
//           kChunk positions, the host walks it
//   tokens  literal: the byte; match: 1 << 31 | (len - 3) << 16 | (dist - 1); then end-of-block
//   codes   makePlan(): code lengths of the block's own histograms (Huffman by the two-queue merge
//           over the symbols sorted by (count, symbol); lengths cut to 15 bits, 7 for the code-length
//           alphabet, by moving leaves down until the Kraft sum fits), canonical codes, and the exact
//           size of the dynamic block.  The code lengths go into the header one by one (the
//           run-length symbols 16 / 17 / 18 are not used)
//   choice  BTYPE 2 unless it would take more bytes than the stored block (5 + m), so a member is
//           never larger than m + 31 bytes
//   CRC32   of slices of kCrcSlice bytes, each brought to the end of the block by a multiplication
//           with x^(8 * bytes after it) mod P, and xor-ed together
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BGZF_HD __host__ __device__ inline
#else
#define BGZF_HD inline
#endif

namespace bgzfblock {

constexpr uint32_t kBlockIn = 0xff00;                 // input bytes per member (host/bam.cpp's split)
constexpr uint32_t kSlot = (kBlockIn + 31 + 15) & ~15u;   // a member's slot: m + 31 bytes at most, 16-byte steps
constexpr uint32_t kDataWords = (kBlockIn + 64) / 4;  // the block (later the member under construction) in words
constexpr uint32_t kHashBits = 13, kTable = 1u << kHashBits;
constexpr uint32_t kWindow = 256, kChunk = 4096;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768, kNear = 4;
constexpr uint32_t kNoCand = 0xffff;                  // no table candidate (a position is below 0xff00)
constexpr uint32_t kLit = 286, kDist = 30, kCl = 19, kEob = 256;
constexpr uint32_t kLitPad = 288, kDistPad = 32;
constexpr uint32_t kCrcSlice = 64, kCrcPoly = 0xedb88320u;
constexpr uint32_t kDeflateBit = 18 * 8;              // the deflate stream follows the 18-byte gzip header

BGZF_HD uint32_t load32(const uint32_t *words, uint32_t p) {
    const uint32_t i = p >> 2, s = (p & 3u) * 8u, lo = words[i];
    return s ? (lo >> s) | (words[i + 1] << (32u - s)) : lo;
}

BGZF_HD uint32_t byteAt(const uint32_t *words, uint32_t p) { return (words[p >> 2] >> ((p & 3u) * 8u)) & 0xffu; }

BGZF_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32u - kHashBits); }

// bytes that data[p ..) and data[q ..) have in common, at most cap (p + cap <= m, q < p)
BGZF_HD uint32_t matchLength(const uint32_t *words, uint32_t p, uint32_t q, uint32_t cap) {
    uint32_t l = 0;
    while (l < cap) {
        const uint32_t x = load32(words, p + l) ^ load32(words, q + l);
        if (x) {
            l += (uint32_t)__builtin_ctz(x) >> 3;
            break;
        }
        l += 4;
    }
    return l < cap ? l : cap;
}

// The match of position p: len 0 for none, else kMinMatch <= len <= kMaxMatch and 1 <= dist <= kMaxDist.
// cand: the table's candidate (kNoCand for none), a position before p's window.
BGZF_HD void bestMatch(const uint32_t *words, uint32_t p, uint32_t m, uint32_t cand, uint32_t &len, uint32_t &dist) {
    len = 0;
    dist = 0;
    if (p + 4 > m) return;
    const uint32_t cap = m - p < kMaxMatch ? m - p : kMaxMatch, v = load32(words, p);
    for (uint32_t d = 1; d <= kNear && d <= p; d++) {
        if (load32(words, p - d) != v) continue;
        const uint32_t l = matchLength(words, p, p - d, cap);
        if (l > len) {
            len = l;
            dist = d;
        }
        if (len == cap) return;
    }
    if (cand != kNoCand && p - cand <= kMaxDist && load32(words, cand) == v) {
        const uint32_t l = matchLength(words, p, cand, cap);
        if (l > len) {
            len = l;
            dist = p - cand;
        }
    }
}

BGZF_HD uint32_t matchToken(uint32_t len, uint32_t dist) { return 0x80000000u | (len - 3u) << 16 | (dist - 1u); }

// RFC 1951 3.2.5: the length symbol of len, its extra bit count and value
BGZF_HD void lenSym(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t l = len - 3u;
    if (len == 258u) { sym = 285; eb = 0; ev = 0; return; }
    if (l < 8u) { sym = 257u + l; eb = 0; ev = 0; return; }
    eb = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    sym = 261u + 4u * eb + ((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
}

BGZF_HD void distSym(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { sym = d; eb = 0; ev = 0; return; }
    eb = (31u - (uint32_t)__builtin_clz(d)) - 1u;
    sym = 2u * eb + 2u + ((d >> eb) & 1u);
    ev = d & ((1u << eb) - 1u);
}

BGZF_HD uint32_t litExtraBits(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) / 4u; }
BGZF_HD uint32_t distExtraBits(uint32_t sym) { return sym < 4u ? 0u : sym / 2u - 1u; }

// ---------------------------------------------------------------- code lengths
struct Scratch {
    uint32_t weight[kLitPad];       // internal nodes, in the order they are made
    uint16_t parent[2 * kLitPad];   // leaves [0, used), then internal nodes
    uint8_t depth[2 * kLitPad];
};

// place of symbol i among the used symbols in ascending (count, symbol) order
BGZF_HD uint32_t rankOf(const uint32_t *freq, uint32_t n, uint32_t i) {
    const uint32_t f = freq[i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t g = freq[j];
        r += g && (g < f || (g == f && j < i));
    }
    return r;
}

// sorted[rank] = symbol for every used symbol -> how many are used
BGZF_HD uint32_t sortSymbols(const uint32_t *freq, uint32_t n, uint16_t *sorted) {
    uint32_t used = 0;
    for (uint32_t i = 0; i < n; i++)
        if (freq[i]) {
            sorted[rankOf(freq, n, i)] = (uint16_t)i;
            used++;
        }
    return used;
}

// Code lengths of n symbols, none above maxBits, unused symbols 0.  One used symbol gets one bit.
BGZF_HD void buildLengths(const uint32_t *freq, uint32_t n, uint32_t maxBits, const uint16_t *sorted, uint32_t used,
                          uint8_t *lens, Scratch &S) {
    for (uint32_t i = 0; i < n; i++) lens[i] = 0;
    if (used == 0) return;
    if (used == 1) {
        lens[sorted[0]] = 1;
        return;
    }
    // two queues: the sorted leaves and the internal nodes, which are made in ascending weight;
    // a leaf goes first when the weights are equal
    uint32_t leaf = 0, node = 0, made = 0;
    while (made < used - 1) {
        uint32_t w = 0;
        for (int k = 0; k < 2; k++) {
            const bool takeLeaf = leaf < used && (node >= made || freq[sorted[leaf]] <= S.weight[node]);
            if (takeLeaf) {
                w += freq[sorted[leaf]];
                S.parent[leaf++] = (uint16_t)(used + made);
            } else {
                w += S.weight[node];
                S.parent[used + node++] = (uint16_t)(used + made);
            }
        }
        S.weight[made++] = w;
    }
    uint32_t count[16];
    for (uint32_t b = 0; b < 16; b++) count[b] = 0;
    const uint32_t root = 2 * used - 2;
    S.depth[root] = 0;
    for (uint32_t i = root; i-- > 0;) {
        const uint32_t d = (uint32_t)S.depth[S.parent[i]] + 1u;
        S.depth[i] = (uint8_t)(d < 255u ? d : 255u);
        if (i < used) count[d < maxBits ? d : maxBits]++;
    }
    // too deep leaves were counted at maxBits: while the Kraft sum is too large, take one leaf from
    // maxBits and split the deepest shorter leaf in two
    uint32_t total = 0;
    for (uint32_t b = 1; b <= maxBits; b++) total += count[b] << (maxBits - b);
    while (total > (1u << maxBits)) {
        count[maxBits]--;
        for (uint32_t b = maxBits - 1; b > 0; b--)
            if (count[b]) {
                count[b]--;
                count[b + 1] += 2;
                break;
            }
        total--;
    }
    // the most frequent symbols take the shortest lengths
    uint32_t j = used;
    for (uint32_t b = 1; b <= maxBits; b++)
        for (uint32_t c = count[b]; c > 0 && j > 0; c--) lens[sorted[--j]] = (uint8_t)b;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed: the stream takes Huffman codes from their top bit
BGZF_HD void canonicalCodes(const uint8_t *lens, uint32_t n, uint16_t *codes) {
    uint32_t count[16], next[16];
    for (uint32_t b = 0; b < 16; b++) count[b] = 0;
    for (uint32_t i = 0; i < n; i++) count[lens[i]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (uint32_t b = 1; b < 16; b++) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = lens[i];
        uint32_t c = l ? next[l]++ : 0u, r = 0;
        for (uint32_t b = 0; b < l; b++, c >>= 1) r = r << 1 | (c & 1u);
        codes[i] = (uint16_t)r;
    }
}

struct Plan {
    uint16_t litCode[kLitPad];
    uint16_t distCode[kDistPad];
    uint16_t clCode[kCl + 1];
    uint8_t litLen[kLitPad];
    uint8_t distLen[kDistPad];
    uint8_t clLen[kCl + 1];
    uint32_t hlit, hdist, hclen;
    uint32_t dynBits;   // bits of the whole dynamic block: header, tokens, end-of-block
};

// litFreq includes the end-of-block symbol.  sortedLit / usedLit: sortSymbols(litFreq, kLit).
BGZF_HD void makePlan(const uint32_t *litFreq, const uint32_t *distFreq, const uint16_t *sortedLit, uint32_t usedLit,
                      Plan &P, Scratch &S) {
    const uint8_t order[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    buildLengths(litFreq, kLit, 15, sortedLit, usedLit, P.litLen, S);
    uint16_t sorted[kDistPad];
    const uint32_t usedDist = sortSymbols(distFreq, kDist, sorted);
    buildLengths(distFreq, kDist, 15, sorted, usedDist, P.distLen, S);
    if (usedDist == 0) P.distLen[0] = 1;   // no match at all: one distance code is still declared
    P.hlit = 257;
    for (uint32_t i = 257; i < kLit; i++)
        if (P.litLen[i]) P.hlit = i + 1;
    P.hdist = 1;
    for (uint32_t i = 1; i < kDist; i++)
        if (P.distLen[i]) P.hdist = i + 1;
    uint32_t clFreq[kCl + 1];
    for (uint32_t i = 0; i <= kCl; i++) clFreq[i] = 0;
    for (uint32_t i = 0; i < P.hlit; i++) clFreq[P.litLen[i]]++;
    for (uint32_t i = 0; i < P.hdist; i++) clFreq[P.distLen[i]]++;
    const uint32_t usedCl = sortSymbols(clFreq, kCl, sorted);
    buildLengths(clFreq, kCl, 7, sorted, usedCl, P.clLen, S);
    if (usedCl == 1) P.clLen[sorted[0] ? 0 : 1] = 1;   // the code-length code must be complete
    P.hclen = 4;
    for (uint32_t i = 4; i < kCl; i++)
        if (P.clLen[order[i]]) P.hclen = i + 1;
    canonicalCodes(P.litLen, kLit, P.litCode);
    canonicalCodes(P.distLen, kDist, P.distCode);
    canonicalCodes(P.clLen, kCl, P.clCode);
    uint32_t bits = 3 + 14 + 3 * P.hclen;
    for (uint32_t i = 0; i < kCl; i++) bits += clFreq[i] * P.clLen[i];
    for (uint32_t i = 0; i < kLit; i++) bits += litFreq[i] * (P.litLen[i] + (i > kEob ? litExtraBits(i) : 0u));
    for (uint32_t i = 0; i < kDist; i++) bits += distFreq[i] * (P.distLen[i] + distExtraBits(i));
    P.dynBits = bits;
}

// ---------------------------------------------------------------- bits
// The n <= 48 bits of v into the stream at bit `at`, low bit first.  O: or(word index, value).
template <class O>
BGZF_HD void orBits(O &o, uint32_t at, uint64_t v, uint32_t n) {
    if (!n) return;
    const uint32_t w = at >> 5, s = at & 31u;
    const uint64_t lo = v << s;
    if ((uint32_t)lo) o.orWord(w, (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) o.orWord(w + 1, (uint32_t)(lo >> 32));
    if (s && s + n > 64u) {
        const uint32_t hi = (uint32_t)(v >> (64u - s));
        if (hi) o.orWord(w + 2, hi);
    }
}

struct PlainOr {   // one writer
    uint32_t *words;
    BGZF_HD void orWord(uint32_t i, uint32_t x) { words[i] |= x; }
};

// the 18 bytes before the deflate stream (host/bam.cpp's header); size: the whole member
template <class O>
BGZF_HD void writeGzipHeader(O &o, uint32_t size) {
    orBits(o, 0, 0x00000004088b1full, 48);        // 31 139 8 4 0 0
    orBits(o, 48, 0x0006ff000000ull, 48);         // 0 0 0 255 6 0
    orBits(o, 96, 0x00024342ull, 32);             // 'B' 'C' 2 0
    orBits(o, 128, size - 1u, 16);
}

// BFINAL, BTYPE 2 and the code lengths -> the bit after them
template <class O>
BGZF_HD uint32_t writeDynamicHeader(O &o, uint32_t at, const Plan &P) {
    const uint8_t order[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    orBits(o, at, 1u | 2u << 1 | (P.hlit - 257u) << 3 | (P.hdist - 1u) << 8 | (P.hclen - 4u) << 13, 17);
    at += 17;
    for (uint32_t i = 0; i < P.hclen; i++, at += 3) orBits(o, at, P.clLen[order[i]], 3);
    for (uint32_t i = 0; i < P.hlit + P.hdist; i++) {
        const uint32_t l = i < P.hlit ? P.litLen[i] : P.distLen[i - P.hlit];
        orBits(o, at, P.clCode[l], P.clLen[l]);
        at += P.clLen[l];
    }
    return at;
}

// the bits of one token
BGZF_HD void tokenBits(uint32_t tok, const Plan &P, uint64_t &bits, uint32_t &n) {
    if (!(tok & 0x80000000u)) {
        bits = P.litCode[tok];
        n = P.litLen[tok];
        return;
    }
    uint32_t sym, eb, ev;
    lenSym(((tok >> 16) & 0xffu) + 3u, sym, eb, ev);
    bits = P.litCode[sym];
    n = P.litLen[sym];
    bits |= (uint64_t)ev << n;
    n += eb;
    distSym((tok & 0x7fffu) + 1u, sym, eb, ev);
    bits |= (uint64_t)P.distCode[sym] << n;
    n += P.distLen[sym];
    bits |= (uint64_t)ev << n;
    n += eb;
}

// ---------------------------------------------------------------- CRC32
BGZF_HD uint32_t crcTableEntry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}

// a * b mod P, polynomials in the CRC's reflected bit order (bit 31 is x^0)
BGZF_HD uint32_t crcMul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1u ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 * 2^k) mod P, k < 16
BGZF_HD uint32_t crcXpow(uint32_t k) {
    uint32_t p = 0x40000000u;   // x^1
    for (uint32_t i = 0; i < k + 3u; i++) p = crcMul(p, p);
    return p;
}

// the CRC32 of len bytes from byte p of the block
BGZF_HD uint32_t crcSlice(const uint32_t *tab, const uint32_t *words, uint32_t p, uint32_t len) {
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < len; i++) c = tab[(c ^ byteAt(words, p + i)) & 0xffu] ^ (c >> 8);
    return ~c;
}

// the CRC32 of a slice as it counts in the CRC32 of the slice followed by `after` more bytes:
// crc(A B) = crcAdvance(crc(A), |B|) ^ crc(B).  xpow[k] = crcXpow(k).
BGZF_HD uint32_t crcAdvance(uint32_t crc, uint32_t after, const uint32_t *xpow) {
    for (uint32_t k = 0; after; k++, after >>= 1)
        if (after & 1u) crc = crcMul(xpow[k], crc);
    return crc;
}

}  // namespace bgzfblock
