// bgzf.cpp -- the host model of the device BGZF compressor (bgzf.hip): snapgpu_bgzf_compress_model.
// One serial loop per block over the steps and functions of bgzf_block.h, blocks spread over the host
// threads, each into its own slot.  Byte-identical to the device stream; needs no GPU and no zlib.
#include "internal.h"
#include "bgzf_block.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

using namespace bgzfblock;

namespace {

const unsigned char kEofBlock[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0,
                                     3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct CrcTables {
    uint32_t tab[256], xpow[16];
    CrcTables() {
        for (uint32_t i = 0; i < 256; i++) tab[i] = crcTableEntry(i);
        for (uint32_t k = 0; k < 16; k++) xpow[k] = crcXpow(k);
    }
};
const CrcTables kCrc;

// what one block needs besides its input: the arrays the device keeps in LDS and its token scratch
struct Work {
    std::vector<uint32_t> data, table, tokens, member;
    std::vector<uint16_t> cand;
    Work() : data(kDataWords), table(kTable), tokens(kBlockIn), member(kDataWords), cand(kBlockIn) {}
};

// One member of m (1 .. kBlockIn) input bytes into out (kSlot bytes) -> its size.
uint32_t modelBlock(const unsigned char *in, uint32_t m, unsigned char *out, Work &W) {
    uint32_t *data = W.data.data();
    std::fill(W.data.begin(), W.data.end(), 0u);
    memcpy(data, in, m);
    // CRC32: slices brought to the end of the block, xor-ed
    uint32_t crc = 0;
    for (uint32_t p = 0; p < m; p += kCrcSlice) {
        const uint32_t len = std::min(kCrcSlice, m - p);
        crc ^= crcAdvance(crcSlice(kCrc.tab, data, p, len), m - p - len, kCrc.xpow);
    }
    // find: windows read the table, then update it
    std::fill(W.table.begin(), W.table.end(), 0u);
    for (uint32_t w0 = 0; w0 < m; w0 += kWindow) {
        const uint32_t w1 = std::min(w0 + kWindow, m);
        for (uint32_t p = w0; p < w1 && p + 4 <= m; p++) {
            const uint32_t c = W.table[hash4(load32(data, p))];
            W.cand[p] = (uint16_t)(c ? c - 1 : kNoCand);
        }
        for (uint32_t p = w0; p < w1 && p + 4 <= m; p++) {
            uint32_t &t = W.table[hash4(load32(data, p))];
            t = std::max(t, p + 1);
        }
    }
    // greedy parse, tokens and histograms
    uint32_t litFreq[kLitPad] = {}, distFreq[kDistPad] = {};
    uint32_t nTok = 0;
    for (uint32_t p = 0; p < m;) {
        uint32_t len, dist;
        bestMatch(data, p, m, W.cand[p], len, dist);
        if (len) {
            uint32_t sym, eb, ev;
            lenSym(len, sym, eb, ev);
            litFreq[sym]++;
            distSym(dist, sym, eb, ev);
            distFreq[sym]++;
            W.tokens[nTok++] = matchToken(len, dist);
            p += len;
        } else {
            const uint32_t b = byteAt(data, p);
            litFreq[b]++;
            W.tokens[nTok++] = b;
            p++;
        }
    }
    litFreq[kEob] = 1;
    Plan P;
    Scratch S;
    uint16_t sortedLit[kLitPad];
    const uint32_t usedLit = sortSymbols(litFreq, kLit, sortedLit);
    makePlan(litFreq, distFreq, sortedLit, usedLit, P, S);
    const uint32_t dynBytes = (P.dynBits + 7) / 8;
    const bool dyn = dynBytes <= 5 + m;
    const uint32_t body = dyn ? dynBytes : 5 + m, size = 18 + body + 8;
    std::fill(W.member.begin(), W.member.end(), 0u);
    PlainOr o{W.member.data()};
    writeGzipHeader(o, size);
    if (dyn) {
        uint32_t at = writeDynamicHeader(o, kDeflateBit, P);
        for (uint32_t i = 0; i < nTok; i++) {
            uint64_t bits;
            uint32_t n;
            tokenBits(W.tokens[i], P, bits, n);
            orBits(o, at, bits, n);
            at += n;
        }
        orBits(o, at, P.litCode[kEob], P.litLen[kEob]);
        at += P.litLen[kEob];
        if (at != kDeflateBit + P.dynBits) return 0;   // the plan's size is exact
    } else {
        orBits(o, kDeflateBit, 1u | (uint64_t)m << 8 | (uint64_t)(~m & 0xffffu) << 24, 40);   // BFINAL, BTYPE 0, LEN, NLEN
    }
    orBits(o, (18 + body) * 8, crc, 32);
    orBits(o, (18 + body) * 8 + 32, m, 32);
    memcpy(out, W.member.data(), size);
    if (!dyn) memcpy(out + 23, in, m);
    return size;
}

}  // namespace

extern "C" int snapgpu_bgzf_compress_model(const char *in, uint64_t n, int eof, char *out, uint64_t cap, uint64_t *used) {
    if ((!in && n) || !used) {
        snapgpu::setError("bgzf_compress_model: null argument");
        return SNAPGPU_EINVAL;
    }
    const uint64_t nBlocks = (n + kBlockIn - 1) / kBlockIn;
    std::vector<unsigned char> slots(nBlocks * kSlot);
    std::vector<uint64_t> at(nBlocks + 1, 0);
    unsigned nt = snapgpu::hostThreads(16);
    if (nBlocks < 4) nt = 1;
    nt = (unsigned)std::min<uint64_t>(nt, std::max<uint64_t>(1, nBlocks));
    auto blocks = [&](uint64_t a, uint64_t b) {
        Work W;
        for (uint64_t k = a; k < b; k++)
            at[k + 1] = modelBlock((const unsigned char *)in + k * kBlockIn, (uint32_t)std::min<uint64_t>(kBlockIn, n - k * kBlockIn),
                                   slots.data() + k * kSlot, W);
    };
    {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(blocks, nBlocks * t / nt, nBlocks * (t + 1) / nt);
        blocks(0, nBlocks / nt);
        for (auto &x : th) x.join();
    }
    for (uint64_t k = 0; k < nBlocks; k++) {
        if (!at[k + 1]) {
            snapgpu::setError("bgzf_compress_model: a block's bits are not the size its code lengths give");
            return SNAPGPU_EIO;
        }
        at[k + 1] += at[k];
    }
    const uint64_t total = at[nBlocks] + (eof ? 28 : 0);
    *used = total;
    if (total > cap || (!out && total)) {
        snapgpu::setError("bgzf_compress_model: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    for (uint64_t k = 0; k < nBlocks; k++) memcpy(out + at[k], slots.data() + k * kSlot, at[k + 1] - at[k]);
    if (eof) memcpy(out + at[nBlocks], kEofBlock, 28);
    return SNAPGPU_OK;
}
