// fastq_record.h -- one FASTQ record as FASTQReader::getNextRead (FASTQ.cpp:196-253) and
// Read::clip (Read.h:357-404) read it, restated over plain pointers for host and device: how a line
// is trimmed, what a record's four lines give, and how qualities clip the read.  The host parser
// (host/reads.cpp), snapgpu_reads_clip (host/sam.cpp) and the device parser (fastq_parse.hip) all
// go through these functions.
//
// As in sam_line.h the rule is a template over a "group" G, the lanes that share one record:
//   g.firstOf(n, pred)     smallest k < n with pred(k), or n
//   g.firstByte(p, n, c)   smallest k < n with p[k] == c, or n
// Serial (below) is one host thread; fastq_parse.hip has the 64-lane wave.  Every member of a
// group calls with the same arguments and receives the same results.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FQ_HD __host__ __device__ inline
#else
#define FQ_HD inline
#endif

namespace fastqrec {

constexpr uint32_t kMinClipped = 50;   // Read::clip: fewer bases left => "just use all of it"

struct Serial {
    template <class P>
    uint64_t firstOf(uint64_t n, P p) const {
        for (uint64_t k = 0; k < n; k++)
            if (p(k)) return k;
        return n;
    }
    uint64_t firstByte(const char *p, uint64_t n, char c) const {
        const void *z = n ? memchr(p, c, n) : nullptr;
        return z ? (uint64_t)((const char *)z - p) : n;
    }
};

// Line [b, e) of text (e: its '\n', or the end of the text): cut at its first NUL byte (the C-string
// reading of the reference's lines), then without its trailing CR / LF bytes.
template <class G>
FQ_HD void trimLine(const char *text, uint64_t b, uint64_t &e, const G &g) {
    e = b + g.firstByte(text + b, e - b, 0);
    const uint64_t end = e;
    e -= g.firstOf(end - b, [=](uint64_t k) { const char c = text[end - 1 - k]; return c != '\r' && c != '\n'; });
}

// A record's trimmed header, bases and quality lines (the '+' line is not read).
struct Record {
    uint64_t idAt, baseAt, qualAt;   // first byte of the id (after '@'), the bases, the qualities
    uint32_t idLen, baseLen, qualLen;
    bool bad;                        // the header line is empty or does not begin with '@'
};

// lineStart(i) / lineEnd(i): line i's first byte and its '\n' (or the end of the text).  A bad
// record's other fields are not set.
template <class G, class B, class E>
FQ_HD Record record(const char *text, uint64_t r, B lineStart, E lineEnd, const G &g) {
    Record R{};
    uint64_t b = lineStart(4 * r), e = lineEnd(4 * r);
    trimLine(text, b, e, g);
    R.bad = e == b || text[b] != '@';
    if (R.bad) return R;
    R.idAt = b + 1;
    R.idLen = (uint32_t)(e - b - 1);
    b = lineStart(4 * r + 1); e = lineEnd(4 * r + 1);
    trimLine(text, b, e, g);
    R.baseAt = b;
    R.baseLen = (uint32_t)(e - b);
    b = lineStart(4 * r + 3); e = lineEnd(4 * r + 3);
    trimLine(text, b, e, g);
    R.qualAt = b;
    R.qualLen = (uint32_t)(e - b);
    return R;
}

// Read::clip over a read's `full` qualities q(0 .. full) (0x00 where the quality line was shorter
// than the bases): the back run of '#' (clipping 2, 3), then the front run (1, 3); fewer than
// kMinClipped bases left => the whole read.
template <class G, class Q>
FQ_HD void clip(Q q, uint32_t full, int clipping, uint32_t &front, uint32_t &len, const G &g) {
    len = full;
    front = 0;
    if (clipping == 2 || clipping == 3)   // ClipBack / ClipFrontAndBack
        len -= (uint32_t)g.firstOf(full, [=](uint64_t k) { return q(full - 1 - k) != '#'; });
    if (clipping == 1 || clipping == 3)   // ClipFront / ClipFrontAndBack
        front = (uint32_t)g.firstOf(len, [=](uint64_t k) { return q(k) != '#'; });
    if (len - front < kMinClipped) { len = full; front = 0; }
    else len -= front;
}

}  // namespace fastqrec
