// bam.cpp -- BAM output of the single-end and RNA paired product paths:
// BAMFormat::writeHeader / writeRead (SNAPLib/Bam.cpp:542-790) over the same per-record fields
// the SAM writer prints (getSAMData, SAM.cpp:804-975), and a BGZF stream (the reference's
// GzipWriterFilter with 64 KB blocks, DataWriterSupplier::gzip(true, 0x10000, ...)).
//
// Kept from the reference: the QNAME is the whole read id (qnameLen, not cut at the first space as
// the SAM text is); SEQ and QUAL cover the whole unclipped read (no "%.*s" NUL stop); an unmapped
// record carries no CIGAR, and its NM is the previous record's (writeRead's editDistance is only
// set when a CIGAR is computed -- the caller passes that value in); bin = reg2bin of the record's
// reference span, (-1, 0) for an unmapped read without mate.
//
// The public host encoder (snapgpu_bam_format, _record_lengths, _sort_keys, _header, snapgpu_bgzf_compress)
// is at the end: records of reads without mate through bam_line.h, the code the device encoder
// (bam_format.hip) compiles too, and records of pairs (snapgpu_bam_format_pairs, _pair_record_lengths,
// _pair_sort_keys) through bam_pair_line.h, which bam_pair_format.hip compiles.
#include "internal.h"
#include "bam_line.h"
#include "bam_pair_line.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

namespace snapgpu {

namespace {

const int SAM_MULTI_SEGMENT = 0x001;       // SAM.h:38-46
const int SAM_ALL_ALIGNED = 0x002;
const int SAM_UNMAPPED = 0x004;
const int SAM_NEXT_UNMAPPED = 0x008;
const int SAM_REVERSE_COMPLEMENT = 0x010;
const int SAM_NEXT_REVERSED = 0x020;
const int SAM_FIRST_SEGMENT = 0x040;
const int SAM_LAST_SEGMENT = 0x080;

inline char upperCase(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 0x20) : c; }
inline char complementOf(char c) {
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': return 'A';
        case 'N': return 'N';
        case 'n': return 'n';
        default: return 0;
    }
}

// BAMAlignment::SeqToCode from CodeToSeq = "=ACMGRSVTWYHKDBN" (Bam.cpp:179, :266-276)
struct SeqCode {
    uint8_t v[256];
    SeqCode() {
        memset(v, 0, sizeof(v));
        const char *c = "=ACMGRSVTWYHKDBN";
        for (int i = 1; i < 16; i++) v[(uint8_t)c[i]] = (uint8_t)i;
    }
};
const SeqCode kSeqCode;
const int kRefBase[16] = {1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};   // CigarCodeToRefBase (Bam.cpp:183)

int reg2bin(int beg, int end) {   // BAMAlignment::reg2bin (Bam.cpp:279-291)
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
    return 0;
}

int pieceAt(const Genome &g, uint32_t loc) {
    int lo = 0, hi = (int)g.pieceOffsets.size() - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) / 2;
        if (g.pieceOffsets[mid] <= loc && (mid == (int)g.pieceOffsets.size() - 1 || g.pieceOffsets[mid + 1] > loc))
            return mid;
        else if (g.pieceOffsets[mid] <= loc) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

template <class T>
void put(std::string &o, T v) { o.append(reinterpret_cast<const char *>(&v), sizeof(T)); }

}  // namespace

// One BAMFormat::writeRead record appended to o (Bam.cpp:596-790): a read without mate, or one end
// of a pair (L.hasMate: getSAMData's mate branch, SAM.cpp:914-973, with piece indices where the SAM
// line has names).  nm: the NM value the reference writes (the record's own edit distance when it
// has a location, else the previous record's).  False if the QNAME is too long for BAM (the
// reference exits, Bam.cpp:723-726).
bool bamAppendRecord(std::string &o, const Genome &g, const SamLine &L, int32_t nm) {
    static const char kOp[] = "MIDNSHP=X";
    uint32_t loc = L.loc;
    if (L.result == SNAPGPU_NOT_FOUND) loc = kInvalidLocation;
    const bool rc = loc != kInvalidLocation && L.dir == SNAPGPU_RC;
    int flags = 0, mapq = 0, pieceIdx = -1;
    uint32_t pos = 0;
    if (loc != kInvalidLocation) {
        if (rc) flags |= SAM_REVERSE_COMPLEMENT;
        const int p = pieceAt(g, loc);
        if (p >= 0) {
            pieceIdx = p;
            pos = loc - g.pieceOffsets[p] + 1;
        }
        mapq = std::max(0, std::min(70, L.mapq));
    } else {
        flags |= SAM_UNMAPPED;
    }
    int mateIdx = -1;
    uint32_t matePos = 0;
    int64_t tlen = 0;
    if (L.hasMate) {
        flags |= SAM_MULTI_SEGMENT | (L.firstInPair ? SAM_FIRST_SEGMENT : SAM_LAST_SEGMENT);
        if (L.mateLoc != kInvalidLocation) {
            const int mp = pieceAt(g, L.mateLoc);
            if (mp >= 0) {
                mateIdx = mp;
                matePos = L.mateLoc - g.pieceOffsets[mp] + 1;
            }
            if (L.mateDir == SNAPGPU_RC) flags |= SAM_NEXT_REVERSED;
            if (loc == kInvalidLocation) {   // the unmapped end takes the mate's RNAME / POS
                pieceIdx = mateIdx;
                pos = matePos;
            }
        } else {                             // the mate is unmapped: it points at this end
            flags |= SAM_NEXT_UNMAPPED;
            mateIdx = pieceIdx;
            matePos = pos;
        }
        if (loc != kInvalidLocation && L.mateLoc != kInvalidLocation) {
            flags |= SAM_ALL_ALIGNED;
            const uint32_t back = L.fullLen - L.clippedLen - L.front;
            const uint32_t before = rc ? back : L.front, after = rc ? L.front : back;
            const int64_t myStart = (int64_t)(uint32_t)(loc - before);
            const int64_t myEnd = (int64_t)(uint32_t)(loc + L.clippedLen + after);
            const int64_t mBefore = L.mateFront, mAfter = (int64_t)L.mateFullLen - L.mateClippedLen - L.mateFront;
            const int64_t mateStart = (int64_t)L.mateLoc - (L.mateDir == SNAPGPU_RC ? mAfter : mBefore);
            const int64_t mateEnd = (int64_t)L.mateLoc + L.mateClippedLen + (L.mateDir == SNAPGPU_FORWARD ? mAfter : mBefore);
            if (pieceIdx >= 0 && pieceIdx == mateIdx) tlen = myStart < mateStart ? mateEnd - myStart : -(myEnd - mateStart);
        }
    }
    const uint32_t qlen = L.qnameLen ? L.qnameLen : L.idLen;
    if (qlen > 254) return false;
    // CIGAR ops: computed at writeRead's own location (even for NotFound), soft clips around them
    std::vector<uint32_t> ops;
    if (L.loc != kInvalidLocation && L.cigar) {   // transcriptome record: insertSpliceJunctions output
        uint32_t num = 0;
        for (char c : *L.cigar) {
            if (c >= '0' && c <= '9') { num = num * 10 + (uint32_t)(c - '0'); continue; }
            const char *k = strchr(kOp, c);
            ops.push_back(num << 4 | (uint32_t)(k ? k - kOp : 0));
            num = 0;
        }
    } else if (L.loc != kInvalidLocation && L.ed >= 0) {
        const uint32_t back = L.fullLen - L.clippedLen - L.front;
        const uint32_t before = rc ? back : L.front, after = rc ? L.front : back;
        if (before) ops.push_back(before << 4 | 4u);
        for (uint32_t k = 0; k < L.nOps; k++) ops.push_back(L.ops[k]);
        if (after) ops.push_back(after << 4 | 4u);
    }
    const uint32_t len = L.fullLen;
    int refLength = ops.empty() ? (int)len : 0;
    for (uint32_t op : ops) refLength += kRefBase[op & 15] * (int)(op >> 4);
    // unmapped: at the mate's position, length 1, or at -1 (Bam.cpp:752-756)
    const int bin = L.loc != kInvalidLocation ? reg2bin((int)pos - 1, (int)pos - 1 + refLength)
                  : (L.hasMate && L.mateLoc != kInvalidLocation) ? reg2bin((int)matePos - 1, (int)matePos)
                                                                  : reg2bin(-1, 0);
    const size_t rgLen = L.rg ? strlen(L.rg) : 0;
    const size_t size = 36 + qlen + 1 + 4 * ops.size() + (len + 1) / 2 + len + (L.rg ? 4 + rgLen : 0) + 8 + 7;
    const size_t start = o.size();
    put<int32_t>(o, (int32_t)(size - 4));                // block_size
    put<int32_t>(o, pieceIdx);                           // refID
    put<int32_t>(o, (int32_t)pos - 1);                   // pos
    put<uint8_t>(o, (uint8_t)(qlen + 1));                // l_read_name
    put<uint8_t>(o, (uint8_t)mapq);                      // MAPQ
    put<uint16_t>(o, (uint16_t)bin);
    put<uint16_t>(o, (uint16_t)ops.size());              // n_cigar_op
    put<uint16_t>(o, (uint16_t)flags);
    put<int32_t>(o, (int32_t)len);                       // l_seq
    put<int32_t>(o, mateIdx);                            // next_refID (-1 without mate)
    put<int32_t>(o, (int32_t)matePos - 1);               // next_pos
    put<int32_t>(o, (int32_t)tlen);                      // tlen
    o.append(L.id, qlen);
    o += '\0';
    for (uint32_t op : ops) put<uint32_t>(o, op);
    // SEQ (4-bit codes) and QUAL (phred) of the unclipped read, reverse-complemented for RC
    std::string seq(len, '\0'), qual(len, '\0');
    for (uint32_t i = 0; i < len; i++) {
        if (rc) {
            seq[i] = complementOf(upperCase(L.bases[len - 1 - i]));
            qual[i] = (char)(L.quals[len - 1 - i] - '!');
        } else {
            seq[i] = upperCase(L.bases[i]);
            qual[i] = (char)(L.quals[i] - '!');
        }
    }
    for (uint32_t i = 0; i + 1 < len; i += 2)
        o += (char)(kSeqCode.v[(uint8_t)seq[i]] << 4 | kSeqCode.v[(uint8_t)seq[i + 1]]);
    if (len % 2) o += (char)(kSeqCode.v[(uint8_t)seq[len - 1]] << 4);
    o += qual;
    if (L.rg) {
        o += "RGZ";
        o.append(L.rg, rgLen);
        o += '\0';
    }
    o.append("PGZSNAP\0", 8);
    o += "NMi";
    put<int32_t>(o, nm);
    return o.size() - start == size;   // block_size must describe exactly what was appended
}

// BAMFormat::writeHeader: magic, the SAM header text, one RefSeq per genome piece with
// l_ref = piece length - 500 (Bam.cpp:542-594)
std::string bamHeader(const Genome &g, const std::string &samText) {
    std::string o("BAM\1", 4);
    put<int32_t>(o, (int32_t)samText.size());
    o += samText;
    const size_t np = g.pieceOffsets.size();
    put<int32_t>(o, (int32_t)np);
    for (size_t i = 0; i < np; i++) {
        const std::string &name = g.pieceNames[i];
        put<int32_t>(o, (int32_t)name.size() + 1);
        o += name;
        o += '\0';
        const uint32_t end = i + 1 < np ? g.pieceOffsets[i + 1] : (uint32_t)g.nBases;
        put<int32_t>(o, (int32_t)((end - g.pieceOffsets[i]) - 500u));
    }
    return o;
}

// BGZF: deflate blocks of at most 0xff00 input bytes, each a gzip member with the BC extra field,
// then the empty EOF block.
static const size_t kBgzfIn = 0xff00;
static const unsigned char kBgzfEof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0,
                                           3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static size_t bgzfBlockBound() { return compressBound(kBgzfIn) + 64; }

// One block of m <= 0xff00 input bytes into out (bgzfBlockBound() bytes) -> its size, 0 on failure.
static size_t bgzfBlock(const char *data, size_t m, unsigned char *out) {
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return 0;
    z.next_in = (Bytef *)data;
    z.avail_in = (uInt)m;
    z.next_out = out + 18;
    z.avail_out = (uInt)(bgzfBlockBound() - 26);
    const int r = deflate(&z, Z_FINISH);
    const size_t clen = z.total_out;
    deflateEnd(&z);
    if (r != Z_STREAM_END) return 0;
    const size_t bsize = 18 + clen + 8;
    const unsigned char hdr[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0,
                                   (unsigned char)((bsize - 1) & 0xff), (unsigned char)((bsize - 1) >> 8)};
    memcpy(out, hdr, 18);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)data, (uInt)m);
    memcpy(out + 18 + clen, &crc, 4);
    const uint32_t isize = (uint32_t)m;
    memcpy(out + 22 + clen, &isize, 4);
    return bsize;
}

bool bgzfWrite(FILE *f, const char *data, size_t n, bool eof) {
    std::vector<unsigned char> out(bgzfBlockBound());
    for (size_t at = 0; at < n; at += kBgzfIn) {
        const size_t bsize = bgzfBlock(data + at, std::min(kBgzfIn, n - at), out.data());
        if (!bsize || fwrite(out.data(), 1, bsize, f) != bsize) return false;
    }
    if (eof && fwrite(kBgzfEof, 1, 28, f) != 28) return false;
    return true;
}

}  // namespace snapgpu

// ------------------------------------------------------------------ the public host encoder
using namespace snapgpu;

namespace {

struct HostRecords {
    samline::Args A;
    std::vector<uint32_t> nameOff;
    std::string names;
};

// The arguments of snapgpu_sam_format_clipped as bam_line.h takes them, checked as the SAM formatter
// checks them, and every QNAME short enough for BAM.
int hostRecordArgs(HostRecords &H, const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                   const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                   const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops, const char *readGroup,
                   const uint32_t *frontClipped, const uint32_t *unclippedLength) {
    if (!idx || !reads || !ids || !idOffsets || !idLengths || !results || !editDistance || !nOps || !ops) {
        setError("bam_format: null argument");
        return SNAPGPU_EINVAL;
    }
    if (int rc = samCheckClips(reads, nOps, &frontClipped, &unclippedLength)) return rc;
    if (int rc = bamCheckIds(idLengths, reads->n)) return rc;
    const Genome &g = *idx->genome;
    samPieceNames(g, H.nameOff, H.names);
    H.A = samline::Args{reads->bases, reads->quals, reads->offsets, reads->lengths, frontClipped, unclippedLength,
                        ids, idOffsets, idLengths, results, editDistance, nOps, ops, g.pieceOffsets.data(),
                        H.nameOff.data(), H.names.data(), (int32_t)g.pieceOffsets.size(),
                        readGroup ? (uint32_t)strlen(readGroup) : 0u, readGroup};
    return SNAPGPU_OK;
}

// f(a, b) over the ranges of [0, n) that the host threads take (one thread below 2 * minPerThread items)
template <class F>
void parallelRanges(uint64_t n, uint64_t minPerThread, F f) {
    unsigned nt = hostThreads(16);
    if (n < minPerThread * 2) nt = 1;
    nt = (unsigned)std::min<uint64_t>(nt, std::max<uint64_t>(1, n));
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back([&, t] { f(n * t / nt, n * (t + 1) / nt); });
    f(0, n / nt);
    for (auto &x : th) x.join();
}

}  // namespace

namespace snapgpu {

int bamCheckIds(const uint32_t *idLengths, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (idLengths[i] > bamline::kMaxQname) {
            setError("bam_format: a read id is longer than 254 bytes (the BAM QNAME limit, Bam.cpp:723-726)");
            return SNAPGPU_EINVAL;
        }
    return SNAPGPU_OK;
}

}  // namespace snapgpu

extern "C" int snapgpu_bam_record_lengths(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                                          const uint64_t *idOffsets, const uint32_t *idLengths,
                                          const snapgpu_result_t *results, const int32_t *editDistance,
                                          const uint32_t *nOps, const uint32_t *ops, const char *readGroup,
                                          const uint32_t *frontClipped, const uint32_t *unclippedLength,
                                          uint32_t *recordLengths) {
    HostRecords H;
    if (int rc = hostRecordArgs(H, idx, reads, ids, idOffsets, idLengths, results, editDistance, nOps, ops, readGroup,
                                frontClipped, unclippedLength))
        return rc;
    if (!recordLengths && reads->n) {
        setError("bam_record_lengths: null argument");
        return SNAPGPU_EINVAL;
    }
    const bamline::Serial g{nullptr};
    for (uint64_t i = 0; i < reads->n; i++) recordLengths[i] = bamline::recordLength(H.A, bamline::fields(H.A, i, g));
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bam_format(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                                  const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                                  const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                  const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                                  int32_t nmCarryIn, int32_t *nmCarryOut, char *out, uint64_t cap, uint64_t *used) {
    if (!used) {
        setError("bam_format: null argument");
        return SNAPGPU_EINVAL;
    }
    HostRecords H;
    if (int rc = hostRecordArgs(H, idx, reads, ids, idOffsets, idLengths, results, editDistance, nOps, ops, readGroup,
                                frontClipped, unclippedLength))
        return rc;
    const uint64_t n = reads->n;
    // sizes and own NM values in parallel, starts and the NM carry on one thread, then every thread
    // writes its records in place
    std::vector<uint64_t> start(n + 1, 0);
    std::vector<int32_t> nm(n);
    const bamline::Serial none{nullptr};
    parallelRanges(n, 4096, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) {
            const bamline::Fields F = bamline::fields(H.A, i, none);
            start[i + 1] = bamline::recordLength(H.A, F);
            nm[i] = F.nmOwn;
        }
    });
    int32_t carry = nmCarryIn;
    for (uint64_t i = 0; i < n; i++) {
        start[i + 1] += start[i];
        if (nm[i] == bamline::kNoNm) nm[i] = carry;
        carry = nm[i];
    }
    if (nmCarryOut) *nmCarryOut = carry;
    *used = start[n];
    if (start[n] > cap || (!out && start[n])) {
        setError("bam_format: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    const bamline::Serial g{out};
    parallelRanges(n, 4096, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; i++) bamline::write(H.A, i, bamline::fields(H.A, i, g), nm[i], start[i], g);
    });
    return SNAPGPU_OK;
}

// The same records through bamAppendRecord, the product paths' encoder, on one host thread: the SamLine
// is built as the SAM formatter builds it (formatOne, sam.cpp).  For tests that pin bam_line.h to it.
extern "C" int snapgpu_internal_bam_append_records(const snapgpu_index_t *idx, const snapgpu_reads_t *reads,
                                                   const char *ids, const uint64_t *idOffsets,
                                                   const uint32_t *idLengths, const snapgpu_result_t *results,
                                                   const int32_t *editDistance, const uint32_t *nOps,
                                                   const uint32_t *ops, const char *readGroup,
                                                   const uint32_t *frontClipped, const uint32_t *unclippedLength,
                                                   int32_t nmCarryIn, int32_t *nmCarryOut, char *out, uint64_t cap,
                                                   uint64_t *used) {
    HostRecords H;
    if (int rc = hostRecordArgs(H, idx, reads, ids, idOffsets, idLengths, results, editDistance, nOps, ops, readGroup,
                                frontClipped, unclippedLength))
        return rc;
    std::string o;
    int32_t nm = nmCarryIn;
    for (uint64_t i = 0; i < reads->n; i++) {
        SamLine L;
        L.id = ids + idOffsets[i];
        L.idLen = idLengths[i];
        L.front = H.A.front ? H.A.front[i] : 0u;
        L.clippedLen = reads->lengths[i];
        L.fullLen = H.A.unclipped ? H.A.unclipped[i] : L.clippedLen;
        L.bases = reads->bases + reads->offsets[i] - L.front;
        L.quals = reads->quals + reads->offsets[i] - L.front;
        L.result = results[i].result;
        L.loc = results[i].location;
        L.dir = results[i].direction;
        L.mapq = results[i].mapq;
        L.ed = editDistance[i];
        L.ops = ops + i * SNAPGPU_CIGAR_MAX_OPS;
        L.nOps = nOps[i];
        L.rg = readGroup;
        if (L.loc != kInvalidLocation && L.ed >= 0) nm = L.ed;
        if (!bamAppendRecord(o, *idx->genome, L, nm)) {
            setError("bam_append_records: record not written");
            return SNAPGPU_EINVAL;
        }
    }
    if (nmCarryOut) *nmCarryOut = nm;
    *used = o.size();
    if (o.size() > cap || !out) {
        setError("bam_append_records: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    memcpy(out, o.data(), o.size());
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bam_sort_keys(const snapgpu_index_t *idx, uint64_t n, const snapgpu_result_t *results,
                                     uint32_t *keys) {
    if (!idx || !idx->genome || ((!results || !keys) && n)) {
        setError("bam_sort_keys: null argument");
        return SNAPGPU_EINVAL;
    }
    const Genome &g = *idx->genome;
    samline::Args A{};
    A.res = results;
    A.pieceOffsets = g.pieceOffsets.data();
    A.nPieces = (int32_t)g.pieceOffsets.size();
    for (uint64_t i = 0; i < n; i++) {
        bamline::Fields F;
        bamline::locate(A, i, F);
        keys[i] = bamline::sortKey(A, F);
    }
    return SNAPGPU_OK;
}

// ------------------------------------------------------------------ pair batches (bam_pair_line.h)
namespace {

struct HostPairRecords {
    samline::PairArgs A;
    std::vector<uint32_t> nameOff;
    std::string names;
};

// The arguments of snapgpu_sam_format_pairs as bam_pair_line.h takes them, checked as the SAM pair
// formatter checks them, and every QNAME short enough for BAM.
int hostPairRecordArgs(HostPairRecords &H, const char *who, const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                       const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results, const int32_t *editDistance,
                       const uint32_t *nOps, const uint32_t *ops, const char *readGroup) {
    if (int rc = samPairArgs(H.A, H.nameOff, H.names, who, idx, reads0, reads1, results, editDistance, nOps, ops, readGroup))
        return rc;
    return bamCheckPairIds(reads0, reads1);
}

}  // namespace

namespace snapgpu {

int bamCheckPairIds(const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1) {
    samline::PairArgs A{};
    const snapgpu_reads_t *R[2] = {reads0, reads1};
    for (int e = 0; e < 2; e++) { A.ids[e] = R[e]->ids; A.idOffsets[e] = R[e]->idOffsets; A.idLengths[e] = R[e]->idLengths; }
    for (uint64_t q = 0; q < reads0->n; q++)
        for (uint32_t e = 0; e < 2; e++)
            if (samline::pairIdLen(A, q, e) > bamline::kMaxQname) {
                setError("bam_format: a read id is longer than 254 bytes (the BAM QNAME limit, Bam.cpp:723-726)");
                return SNAPGPU_EINVAL;
            }
    return SNAPGPU_OK;
}

}  // namespace snapgpu

extern "C" int snapgpu_bam_pair_record_lengths(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                               const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results,
                                               const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                               const char *readGroup, uint32_t *recordLengths) {
    HostPairRecords H;
    if (int rc = hostPairRecordArgs(H, "bam_pair_record_lengths", idx, reads0, reads1, results, editDistance, nOps, ops, readGroup))
        return rc;
    if (!recordLengths && reads0->n) {
        setError("bam_pair_record_lengths: null argument");
        return SNAPGPU_EINVAL;
    }
    const bampairline::Serial g{nullptr};
    for (uint64_t j = 0; j < 2 * reads0->n; j++)
        recordLengths[j] = bampairline::recordLength(H.A, bampairline::fields(H.A, j, g));
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bam_format_pairs(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                        const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results,
                                        const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                        const char *readGroup, int32_t nmCarryIn, int32_t *nmCarryOut, char *out,
                                        uint64_t cap, uint64_t *used) {
    if (!used) {
        setError("bam_format_pairs: null argument");
        return SNAPGPU_EINVAL;
    }
    *used = 0;
    HostPairRecords H;
    if (int rc = hostPairRecordArgs(H, "bam_format_pairs", idx, reads0, reads1, results, editDistance, nOps, ops, readGroup))
        return rc;
    const uint64_t recs = 2 * reads0->n;
    // sizes and own NM values in parallel, starts and the NM carry on one thread in write order (the
    // record order), then every thread writes its records in place
    std::vector<uint64_t> start(recs + 1, 0);
    std::vector<int32_t> nm(recs);
    const bampairline::Serial none{nullptr};
    parallelRanges(recs, 4096, [&](uint64_t a, uint64_t b) {
        for (uint64_t j = a; j < b; j++) {
            const bampairline::Fields F = bampairline::fields(H.A, j, none);
            start[j + 1] = bampairline::recordLength(H.A, F);
            nm[j] = F.nmOwn;
        }
    });
    int32_t carry = nmCarryIn;
    for (uint64_t j = 0; j < recs; j++) {
        start[j + 1] += start[j];
        if (nm[j] == bampairline::kNoNm) nm[j] = carry;
        carry = nm[j];
    }
    if (nmCarryOut) *nmCarryOut = carry;
    *used = start[recs];
    if (start[recs] > cap || (!out && start[recs])) {
        setError("bam_format_pairs: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    const bampairline::Serial g{out};
    parallelRanges(recs, 4096, [&](uint64_t a, uint64_t b) {
        for (uint64_t j = a; j < b; j++) bampairline::write(H.A, j, bampairline::fields(H.A, j, g), nm[j], start[j], g);
    });
    return SNAPGPU_OK;
}

// The same records through bamAppendRecord with SamLine::hasMate, the RNA paired path's encoder, on
// one host thread: the NM pass and the SamLine as host/rna_paired.cpp's record loop has them (without
// transcriptome CIGARs).  For tests that pin bam_pair_line.h to it.
extern "C" int snapgpu_internal_bam_append_pair_records(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                                        const snapgpu_reads_t *reads1,
                                                        const snapgpu_pair_result_t *results,
                                                        const int32_t *editDistance, const uint32_t *nOps,
                                                        const uint32_t *ops, const char *readGroup, int32_t nmCarryIn,
                                                        int32_t *nmCarryOut, char *out, uint64_t cap, uint64_t *used) {
    if (!used) return SNAPGPU_EINVAL;
    *used = 0;
    HostPairRecords H;
    if (int rc = hostPairRecordArgs(H, "bam_append_pair_records", idx, reads0, reads1, results, editDistance, nOps, ops, readGroup))
        return rc;
    const samline::PairArgs &A = H.A;
    std::string o;
    int32_t lastNm = nmCarryIn;
    for (uint64_t q = 0; q < reads0->n; q++) {
        const snapgpu_pair_result_t &r = A.res[q];
        uint32_t idLen[2] = {A.idLengths[0][q], A.idLengths[1][q]};
        const char *id[2] = {A.ids[0] + A.idOffsets[0][q], A.ids[1] + A.idOffsets[1][q]};
        if (idLen[0] == idLen[1] && idLen[0] > 2 && id[0][idLen[0] - 2] == '/' && id[1][idLen[0] - 2] == '/') {
            const char c0 = id[0][idLen[0] - 1], c1 = id[1][idLen[1] - 1];
            if ((c0 == '1' || c0 == '2') && (c0 == '1' || c1 == '2') && c0 != c1) { idLen[0] -= 2; idLen[1] -= 2; }
        }
        uint32_t locs[2];
        for (int k = 0; k < 2; k++) locs[k] = r.status[k] != SNAPGPU_NOT_FOUND ? r.location[k] : kInvalidLocation;
        const int first = locs[0] > locs[1], second = 1 - first;
        for (int w = 0; w < 2; w++) {
            const int k = w == 0 ? first : second, m = 1 - k;
            SamLine L;
            L.id = id[k];
            L.idLen = A.idLengths[k][q];
            L.qnameLen = idLen[k];
            L.front = A.front[k] ? A.front[k][q] : 0u;
            L.clippedLen = A.lengths[k][q];
            L.fullLen = A.unclipped[k] ? A.unclipped[k][q] : L.clippedLen;
            L.bases = A.bases[k] + A.offsets[k][q] - L.front;
            L.quals = A.quals[k] + A.offsets[k][q] - L.front;
            L.rg = A.rg;
            L.result = r.status[k];
            L.loc = locs[k];
            L.dir = r.direction[k];
            L.mapq = r.mapq[k];
            L.ed = A.ed[2 * q + k];
            L.ops = A.ops + (2 * q + k) * SNAPGPU_CIGAR_MAX_OPS;
            L.nOps = A.nOps[2 * q + k];
            L.hasMate = true;
            L.firstInPair = w == 0;
            L.mateLoc = locs[m];
            L.mateDir = r.direction[m];
            L.mateFront = A.front[m] ? A.front[m][q] : 0u;
            L.mateClippedLen = A.lengths[m][q];
            L.mateFullLen = A.unclipped[m] ? A.unclipped[m][q] : L.mateClippedLen;
            if (locs[k] != kInvalidLocation) lastNm = L.ed;
            if (!bamAppendRecord(o, *idx->genome, L, lastNm)) {
                setError("bam_append_pair_records: record not written");
                return SNAPGPU_EINVAL;
            }
        }
    }
    if (nmCarryOut) *nmCarryOut = lastNm;
    *used = o.size();
    if (o.size() > cap || !out) {
        setError("bam_append_pair_records: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    memcpy(out, o.data(), o.size());
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bam_pair_sort_keys(const snapgpu_index_t *idx, uint64_t n, const snapgpu_pair_result_t *results,
                                          uint32_t *keys) {
    if (!idx || !idx->genome || ((!results || !keys) && n)) {
        setError("bam_pair_sort_keys: null argument");
        return SNAPGPU_EINVAL;
    }
    const Genome &g = *idx->genome;
    samline::PairArgs A{};
    A.res = results;
    A.pieceOffsets = g.pieceOffsets.data();
    A.nPieces = (int32_t)g.pieceOffsets.size();
    for (uint64_t j = 0; j < 2 * n; j++) {
        samline::PairFields P;
        bampairline::Fields F;
        bampairline::place(A, j, P, F);
        keys[j] = bampairline::sortKey(A, F);
    }
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bam_header(const snapgpu_index_t *idx, const char *samHeaderText, uint64_t n, char *out,
                                  uint64_t cap, uint64_t *used) {
    if (!idx || !idx->genome || (!samHeaderText && n) || !used) {
        setError("bam_header: null argument");
        return SNAPGPU_EINVAL;
    }
    const std::string o = bamHeader(*idx->genome, std::string(samHeaderText ? samHeaderText : "", n));
    *used = o.size();
    if (o.size() > cap || !out) {
        setError("bam_header: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    memcpy(out, o.data(), o.size());
    return SNAPGPU_OK;
}

extern "C" int snapgpu_bgzf_compress(const char *in, uint64_t n, int eof, char *out, uint64_t cap, uint64_t *used) {
    if ((!in && n) || !used) {
        setError("bgzf_compress: null argument");
        return SNAPGPU_EINVAL;
    }
    // every block is its own deflate stream: blocks are compressed on the host threads, each into
    // its own slot, and concatenated in order -- the bytes do not depend on the thread count
    const uint64_t nBlocks = (n + kBgzfIn - 1) / kBgzfIn;
    const size_t slot = bgzfBlockBound();
    std::vector<unsigned char> slots(nBlocks * slot);
    std::vector<uint64_t> at(nBlocks + 1, 0);
    parallelRanges(nBlocks, 2, [&](uint64_t a, uint64_t b) {
        for (uint64_t k = a; k < b; k++)
            at[k + 1] = bgzfBlock(in + k * kBgzfIn, (size_t)std::min<uint64_t>(kBgzfIn, n - k * kBgzfIn), slots.data() + k * slot);
    });
    for (uint64_t k = 0; k < nBlocks; k++) {
        if (!at[k + 1]) {
            setError("bgzf_compress: deflate failed");
            return SNAPGPU_EIO;
        }
        at[k + 1] += at[k];
    }
    const uint64_t total = at[nBlocks] + (eof ? 28 : 0);
    *used = total;
    if (total > cap || (!out && total)) {
        setError("bgzf_compress: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    parallelRanges(nBlocks, 2, [&](uint64_t a, uint64_t b) {
        for (uint64_t k = a; k < b; k++) memcpy(out + at[k], slots.data() + k * slot, at[k + 1] - at[k]);
    });
    if (eof) memcpy(out + at[nBlocks], kBgzfEof, 28);
    return SNAPGPU_OK;
}
