// inflate.cpp -- BGZF streams inflated on the host: the member walk every form shares (bgzfWalk),
// snapgpu_bgzf_inflate (zlib, members spread over the host threads: snapgpu_bgzf_compress's
// counterpart) and snapgpu_bgzf_inflate_model (the same through inflate_block.h, the code the
// device kernel of inflate.hip compiles; needs no GPU and no zlib).
#include "internal.h"
#include "inflate_block.h"

#include <zlib.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

using namespace inflateblock;

namespace snapgpu {

namespace {

uint32_t le16(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
uint32_t le32(const unsigned char *p) { return le16(p) | le16(p + 2) << 16; }

int walkError(const char *what, uint64_t index, uint64_t at, const char *why) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: member %llu at byte %llu: %s", what, (unsigned long long)index, (unsigned long long)at, why);
    setError(msg);
    return SNAPGPU_EFORMAT;
}

}  // namespace

int bgzfWalk(const char *what, const char *data, uint64_t n, std::vector<Member> &members, uint64_t *outBytes) {
    const unsigned char *in = (const unsigned char *)data;
    members.clear();
    uint64_t at = 0, out = 0;
    while (at < n) {
        const uint64_t k = members.size();
        if (n - at < 12) return walkError(what, k, at, "fewer bytes than a gzip header");
        const unsigned char *h = in + at;
        if (h[0] != 0x1f || h[1] != 0x8b) return walkError(what, k, at, "no gzip magic");
        if (h[2] != 8) return walkError(what, k, at, "compression method is not deflate");
        if (h[3] != 4) return walkError(what, k, at, "gzip, but not BGZF: FLG is not 4 (no extra field alone)");
        const uint32_t xlen = le16(h + 10);
        if (n - at - 12 < xlen) return walkError(what, k, at, "the extra field passes the end of the stream");
        bool found = false;
        uint32_t bsize = 0, p = 0;
        while (p + 4 <= xlen) {
            const unsigned char *f = h + 12 + p;
            const uint32_t slen = le16(f + 2);
            if (slen > xlen - p - 4) return walkError(what, k, at, "a subfield passes the end of the extra field");
            if (!found && f[0] == 'B' && f[1] == 'C' && slen == 2) {
                found = true;
                bsize = le16(f + 4);
            }
            p += 4 + slen;
        }
        if (p != xlen) return walkError(what, k, at, "the extra field does not end with a subfield");
        if (!found) return walkError(what, k, at, "gzip, but not BGZF: no BC subfield with the member's size");
        const uint64_t size = (uint64_t)bsize + 1;
        if (size < 12ull + xlen + 8) return walkError(what, k, at, "BSIZE is smaller than header and trailer");
        if (size > n - at) return walkError(what, k, at, "BSIZE passes the end of the stream");
        const uint32_t isize = le32(h + size - 4);
        if (isize > kMaxOut) return walkError(what, k, at, "ISIZE is larger than 65,536");
        members.push_back(Member{at, out, (uint32_t)size, isize, 12 + xlen, 0});
        at += size;
        out += isize;
    }
    *outBytes = out;
    return SNAPGPU_OK;
}

int bgzfRefused(const char *what, uint64_t index, uint64_t at, uint32_t status) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: member %llu at byte %llu: %s (status %u)", what, (unsigned long long)index,
             (unsigned long long)at, statusName(status), status);
    setError(msg);
    return SNAPGPU_EFORMAT;
}

namespace {

struct CrcTables {
    uint32_t tab[256], xpow[16];
    CrcTables() {
        for (uint32_t i = 0; i < 256; i++) tab[i] = bgzfblock::crcTableEntry(i);
        for (uint32_t k = 0; k < 16; k++) xpow[k] = bgzfblock::crcXpow(k);
    }
};
const CrcTables kCrc;

// zlib over one member, straight into its place -> a Status (only ok / not ok matter to the caller's message)
uint32_t zlibMember(const unsigned char *in, const Member &M, unsigned char *dst) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return kInputExhausted;
    unsigned char none = 0;
    z.next_in = const_cast<unsigned char *>(in + M.inStart + M.defOff);
    z.avail_in = M.inSize - M.defOff - 8;
    z.next_out = M.outSize ? dst : &none;   // an empty member: room for the byte it must not write
    z.avail_out = M.outSize ? M.outSize : 1;
    const int r = inflate(&z, Z_FINISH);
    const bool all = z.avail_in == 0;
    const uint64_t got = z.total_out;
    inflateEnd(&z);
    if (r != Z_STREAM_END) return kNoCode;
    if (!all) return kTrailingBytes;
    if (got != M.outSize) return kSizeMismatch;
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, M.outSize);
    return crc == le32(in + M.inStart + M.inSize - 8) ? kOk : kCrcMismatch;
}

uint32_t modelMember(const unsigned char *in, const Member &M, unsigned char *dst, Work &W) {
    const unsigned char *def = in + M.inStart + M.defOff;
    const uint32_t n = M.inSize - M.defOff - 8;
    const uint32_t st = inflateMember(def, n, M.outSize, le32(def + n), W, Serial{});
    if (st == kOk && M.outSize) memcpy(dst, W.win, M.outSize);
    return st;
}

int inflateHost(const char *what, bool model, const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used) {
    if ((!in && n) || !used) {
        setError(std::string(what) + ": null argument");
        return SNAPGPU_EINVAL;
    }
    *used = 0;
    std::vector<Member> members;
    uint64_t total = 0;
    if (int rc = bgzfWalk(what, in, n, members, &total)) return rc;
    *used = total;
    if (total > cap || (!out && total)) {
        setError(std::string(what) + ": output buffer too small");
        return SNAPGPU_EINVAL;
    }
    const uint64_t nm = members.size();
    std::vector<uint32_t> status(nm, 0);
    unsigned nt = hostThreads(16);
    if (nm < 4) nt = 1;
    nt = (unsigned)std::min<uint64_t>(nt, std::max<uint64_t>(1, nm));
    auto run = [&](uint64_t a, uint64_t b) {
        std::unique_ptr<Work> W;
        if (model) {
            W.reset(new Work);
            memcpy(W->crcTab, kCrc.tab, sizeof kCrc.tab);
            memcpy(W->xpow, kCrc.xpow, sizeof kCrc.xpow);
        }
        for (uint64_t k = a; k < b; k++) {
            unsigned char *dst = (unsigned char *)out + members[k].outStart;
            status[k] = model ? modelMember((const unsigned char *)in, members[k], dst, *W)
                              : zlibMember((const unsigned char *)in, members[k], dst);
        }
    };
    {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(run, nm * t / nt, nm * (t + 1) / nt);
        run(0, nm / nt);
        for (auto &x : th) x.join();
    }
    for (uint64_t k = 0; k < nm; k++)   // the lowest bad member, whichever thread met it
        if (status[k]) {
            if (model) return bgzfRefused(what, k, members[k].inStart, status[k]);
            char msg[200];
            snprintf(msg, sizeof msg, "%s: member %llu at byte %llu: zlib does not give ISIZE bytes with the trailer's CRC32",
                     what, (unsigned long long)k, (unsigned long long)members[k].inStart);
            setError(msg);
            return SNAPGPU_EFORMAT;
        }
    return SNAPGPU_OK;
}

}  // namespace

}  // namespace snapgpu

extern "C" int snapgpu_bgzf_inflate_size(const char *in, uint64_t n, uint64_t *outBytes, uint64_t *nMembers) {
    if ((!in && n) || !outBytes || !nMembers) {
        snapgpu::setError("bgzf_inflate_size: null argument");
        return SNAPGPU_EINVAL;
    }
    *outBytes = *nMembers = 0;
    std::vector<Member> members;
    uint64_t total = 0;
    if (int rc = snapgpu::bgzfWalk("bgzf_inflate_size", in, n, members, &total)) return rc;
    *outBytes = total;
    *nMembers = members.size();
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bgzf_inflate(const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used) {
    return snapgpu::inflateHost("bgzf_inflate", false, in, n, out, cap, used);
}

extern "C" int snapgpu_bgzf_inflate_model(const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used) {
    return snapgpu::inflateHost("bgzf_inflate_model", true, in, n, out, cap, used);
}
