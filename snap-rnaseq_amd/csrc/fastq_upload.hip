// fastq_upload.hip -- the host side of the resident input chain behind include/snapgpu.h: FASTQ
// parsed on the device into a resident read batch (fastq_parse.hip), from plain text or from a
// BGZF stream inflated on the device (inflate.hip), and what a caller reads back from such a batch.
// No kernels here.  The state types are in aligner_state.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "aligner_state.h"
#include "fastq_parse.h"
#include "inflate.h"

using namespace sgk;

namespace {

const uint64_t kFastqChunk = 16ull << 20;   // bytes per pinned staging chunk of the text upload

// hipMemGetInfo before a group of allocations, as the device index builder asks: the group must fit
// in what is free now.
int fqFits(uint64_t need, const char *what) {
    size_t freeB = 0, totalB = 0;
    HIPCHK(hipMemGetInfo(&freeB, &totalB));
    if (need > freeB) {
        char msg[200];
        snprintf(msg, sizeof msg, "fastq_upload: %s needs %llu bytes of device memory, %llu are free", what,
                 (unsigned long long)need, (unsigned long long)freeB);
        snapgpu::setError(msg);
        return SNAPGPU_ENOMEM;
    }
    return SNAPGPU_OK;
}

// fill(dst, off, m): bytes [off, off + m) of the text into a staging chunk (false: setError was called)
using FastqFill = std::function<bool(char *, uint64_t, uint64_t)>;

// nBytes of text (or of a compressed stream) to dst[0 .. cap) in device memory, zeros after them,
// through two pinned staging chunks: chunk k + 1 is filled by the host while chunk k crosses PCIe
// (textDownload's reverse).  *last = the last byte.
int fastqTextUpload(snapgpu_aligner_t *a, char *dst, uint64_t cap, uint64_t nBytes, const FastqFill &fill, char *last) {
    auto &F = a->fq;
    for (int k = 0; k < 2; k++) {
        if (!F.pin[k]) HIPCHK(hipHostMalloc(&F.pin[k], kFastqChunk, hipHostMallocDefault));
        if (!F.pinDone[k]) HIPCHK(hipEventCreateWithFlags(&F.pinDone[k], hipEventDisableTiming));
    }
    HIPCHK(hipMemsetAsync(dst + nBytes, 0, cap - nBytes, a->copyStream));
    const uint64_t nChunks = (nBytes + kFastqChunk - 1) / kFastqChunk;
    for (uint64_t k = 0; k < nChunks; k++) {
        const uint64_t b = k * kFastqChunk, m = std::min(kFastqChunk, nBytes - b);
        char *pin = (char *)F.pin[k & 1];
        if (k >= 2)
            if (int rc = waitEvent(a, F.pinDone[k & 1])) return rc;
        if (!fill(pin, b, m)) return SNAPGPU_EIO;
        if (k + 1 == nChunks) *last = pin[m - 1];
        HIPCHK(hipMemcpyAsync(dst + b, pin, m, hipMemcpyHostToDevice, a->copyStream));
        HIPCHK(hipEventRecord(F.pinDone[k & 1], a->copyStream));
    }
    HIPCHK(hipStreamSynchronize(a->copyStream));
    return SNAPGPU_OK;
}

// [0, m) split over this rank's host threads (one below 1 MB)
template <class Fn>
void fastqParallel(uint64_t m, Fn fn) {
    const unsigned t = m < (1u << 20) ? 1u : snapgpu::hostThreads(16);
    std::vector<std::thread> th;
    for (unsigned j = 1; j < t; j++) th.emplace_back([=] { fn(m * j / t, m * (j + 1) / t); });
    fn(0, m / t);
    for (auto &x : th) x.join();
}

// ---- BGZF inflated on the device (inflate.hip)
using inflateblock::Member;

int inflateWaves(snapgpu_aligner_t *a) {
    if (!a->inf.waves) {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, a->device));
        a->inf.waves = std::max(1, prop.multiProcessorCount) * (int)inflategpu::kWavesPerCu;
    }
    return SNAPGPU_OK;
}

// what the inflater's own buffers would newly allocate for a stream of n bytes in nMembers members
uint64_t inflateGrowBytes(const snapgpu_aligner_t *a, uint64_t n, uint64_t nMembers) {
    return growBytes(a->inf.in, n + inflategpu::kInSlack) + growBytes(a->inf.members, nMembers * sizeof(Member) + 16) +
           growBytes(a->inf.status, (nMembers + 1) * 4 + 16);
}

// The stream to device memory through the text upload's staging chunks, its member table beside
// it, the kernel over all members into dst (device memory with room for every member's output),
// and the verdict: SNAPGPU_EFORMAT with the lowest refused member.  The caller has checked
// inflateGrowBytes and dst against the device's free memory.  Waits.
int inflateOnDevice(snapgpu_aligner_t *a, const char *what, const char *in, uint64_t n, const std::vector<Member> &members,
                    char *dst) {
    using clk = std::chrono::steady_clock;
    auto &I = a->inf;
    I.ran = false;
    I.uploadMs = I.kernelMs = I.downloadMs = 0;
    const uint64_t nm = members.size();
    if (nm >= inflategpu::kNoBad) { snapgpu::setError(std::string(what) + ": too many members"); return SNAPGPU_EINVAL; }
    if (int rc = inflateWaves(a)) return rc;
    for (auto &e : I.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(devGrow(a, I.in, n + inflategpu::kInSlack));
    HIPCHK(devGrow(a, I.members, nm * sizeof(Member) + 16));
    HIPCHK(devGrow(a, I.status, (nm + 1) * 4 + 16));
    auto t0 = clk::now();
    const FastqFill fill = [in](char *pin, uint64_t off, uint64_t m) {
        fastqParallel(m, [=](uint64_t b, uint64_t e) { memcpy(pin + b, in + off + b, e - b); });
        return true;
    };
    char last = 0;
    if (int rc = fastqTextUpload(a, (char *)I.in.p, n + inflategpu::kInSlack, n, fill, &last)) return rc;
    if (nm) HIPCHK(hipMemcpyAsync(I.members.p, members.data(), nm * sizeof(Member), hipMemcpyHostToDevice, a->copyStream));
    HIPCHK(hipStreamSynchronize(a->copyStream));
    I.uploadMs = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    hipStream_t s = a->stream();
    uint32_t *status = (uint32_t *)I.status.p, *firstBad = status + nm;
    HIPCHK(hipEventRecord(I.ev[0], s));
    HIPCHK(inflategpu::launch((const uint8_t *)I.in.p, (const Member *)I.members.p, (uint32_t)nm, (uint8_t *)dst, status,
                              firstBad, (uint32_t)I.waves, s));
    HIPCHK(hipEventRecord(I.ev[1], s));
    uint32_t bad = inflategpu::kNoBad;
    HIPCHK(hipMemcpyAsync(&bad, firstBad, 4, hipMemcpyDeviceToHost, s));
    if (int rc = waitLane(a, a->lane[0])) return rc;
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, I.ev[0], I.ev[1]));
    I.kernelMs = f;
    I.ran = true;
    if (bad != inflategpu::kNoBad) {
        if (bad >= nm) { snapgpu::setError(std::string(what) + ": the kernel names a member the stream does not have"); return SNAPGPU_EDEVICE; }
        uint32_t st = 0;
        HIPCHK(hipMemcpy(&st, status + bad, 4, hipMemcpyDeviceToHost));
        return snapgpu::bgzfRefused(what, bad, members[bad].inStart, st);
    }
    return SNAPGPU_OK;
}

// How the text reaches the parser's device buffer, which fastqRun sizes: the plain form uploads it
// (fastqTextUpload), the BGZF form uploads the compressed stream and inflates it there.
struct FastqArrival {
    uint64_t nBytes = 0;      // the text's bytes
    uint64_t extraNeed = 0;   // device bytes the arrival itself newly allocates (fastqRun's memory check counts them)
    // the text into text[0 .. nBytes), zeros from there to cap; *last = its last byte (nBytes > 0);
    // *kernelMs = what its own kernels took
    std::function<int(char *text, uint64_t cap, char *last, double *kernelMs)> arrive;
};

// d and r: what the call has allocated so far (the caller frees them when the call fails)
int fastqRun(snapgpu_aligner_t *a, const FastqArrival &arrival, const char *name, int clipping, bool hostBatch,
             snapgpu_device_reads_t *&d, snapgpu_reads_t *&r) {
    const uint64_t nBytes = arrival.nBytes;
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    auto &F = a->fq;
    hipStream_t s = a->stream(), cs = a->copyStream;
    for (auto &e : F.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    F.ran = false;
    F.uploadMs = F.kernelMs = F.downloadMs = F.arriveKernelMs = 0;
    for (double &m : F.passMs) m = 0;
    bool evUsed[3] = {false, false, false};
    // 1. the text, its tiles' newline counts and their scan
    const uint64_t nTiles = fqgpu::tiles(nBytes), textCap = fqgpu::textCapacity(nBytes);
    const uint64_t needTiles[4] = {textCap, nTiles * 4 + 16, (nTiles + 1) * 8, samgpu::scanTiles(nTiles) * 8 + 16};
    DevBuf *bufTiles[4] = {&F.text, &F.counts, &F.tileStart, &F.sums};
    uint64_t need = arrival.extraNeed;
    for (int k = 0; k < 4; k++) need += growBytes(*bufTiles[k], needTiles[k]);
    if (int rc = fqFits(need, "the text")) return rc;
    for (int k = 0; k < 4; k++) HIPCHK(devGrow(a, *bufTiles[k], needTiles[k]));
    const char *text = (const char *)F.text.p;
    char last = '\n';
    auto t0 = clk::now();
    if (int rc = arrival.arrive((char *)F.text.p, textCap, &last, &F.arriveKernelMs)) return rc;
    F.uploadMs = ms(t0) - F.arriveKernelMs;
    uint64_t nNl = 0;
    if (nBytes) {
        HIPCHK(hipEventRecord(F.ev[0], s));
        fqgpu::countNewlines(text, nBytes, (uint32_t *)F.counts.p, s);
        HIPCHK(hipEventRecord(F.ev[1], s));
        samgpu::scanStarts((const uint32_t *)F.counts.p, nTiles, (uint64_t *)F.sums.p, (uint64_t *)F.tileStart.p, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(F.ev[2], s));
        evUsed[0] = true;
        HIPCHK(hipMemcpyAsync(&nNl, (const uint64_t *)F.tileStart.p + nTiles, 8, hipMemcpyDeviceToHost, s));
        if (int rc = waitLane(a, a->lane[0])) return rc;
    }
    // records are the line quadruples; a last line without its newline counts
    const uint64_t nLines = nNl + (nBytes && last != '\n' ? 1 : 0), n = nLines / 4;
    if (n > 0xffffffffull) { snapgpu::setError("fastq_upload: batch too large"); return SNAPGPU_EINVAL; }
    // 2. newline positions, the records' lengths and clips, the scans of base and id lengths
    uint64_t total = 0, idTotal = 0;
    fqgpu::Records R{};
    fqgpu::Totals hTot{};
    if (n) {
        const uint64_t needRec[7] = {nNl * 8 + 16, n * 20 + 16, (n + 1) * 8, (n + 1) * 8, samgpu::scanTiles(n) * 8 + 16,
                                     samgpu::scanTiles(n) * 8 + 16, sizeof(fqgpu::Totals)};
        DevBuf *bufRec[7] = {&F.nl, &F.rec, &F.baseStart, &F.idStart, &F.sums, &F.sums2, &F.tot};
        need = 0;
        for (int k = 0; k < 7; k++) need += growBytes(*bufRec[k], needRec[k]);
        if (int rc = fqFits(need, "the line and record arrays")) return rc;
        for (int k = 0; k < 7; k++) HIPCHK(devGrow(a, *bufRec[k], needRec[k]));
        uint32_t *rec = (uint32_t *)F.rec.p;
        R = fqgpu::Records{rec, rec + n, rec + 2 * n, rec + 3 * n, rec + 4 * n};
        auto *tot = (fqgpu::Totals *)F.tot.p;
        HIPCHK(hipEventRecord(F.ev[3], s));
        HIPCHK(hipMemsetAsync(&tot->firstBad, 0xff, 8, s));
        HIPCHK(hipMemsetAsync(&tot->baseBytes, 0, 16, s));   // and the two maxima behind it
        fqgpu::lineStarts(text, nBytes, (const uint64_t *)F.tileStart.p, (uint64_t *)F.nl.p, nNl, s);
        HIPCHK(hipEventRecord(F.ev[4], s));
        fqgpu::records(text, nBytes, (const uint64_t *)F.nl.p, nNl, n, clipping, R, tot, s);
        HIPCHK(hipEventRecord(F.ev[5], s));
        samgpu::scanStarts(R.baseLen, n, (uint64_t *)F.sums.p, (uint64_t *)F.baseStart.p, s);
        samgpu::scanStarts(R.idLen, n, (uint64_t *)F.sums2.p, (uint64_t *)F.idStart.p, s);
        fqgpu::limits(R.baseLen, R.idLen, n, tot, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(F.ev[6], s));
        evUsed[1] = true;
        HIPCHK(hipMemcpyAsync(&hTot, tot, sizeof hTot, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&total, (const uint64_t *)F.baseStart.p + n, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&idTotal, (const uint64_t *)F.idStart.p + n, 8, hipMemcpyDeviceToHost, s));
        if (int rc = waitLane(a, a->lane[0])) return rc;
        if (hTot.firstBad < n) {
            snapgpu::setError(std::string("FASTQ record without '@' header in ") + name);
            return SNAPGPU_EFORMAT;
        }
        if (hTot.baseBytes != total) {
            char msg[160];
            snprintf(msg, sizeof msg, "fastq_upload: the record pass counted %llu base bytes, the scan placed %llu",
                     (unsigned long long)hTot.baseBytes, (unsigned long long)total);
            snapgpu::setError(msg);
            return SNAPGPU_EDEVICE;
        }
    }
    // 3. the resident batch (snapgpu_reads_upload's buffers) and the copy pass into it
    const uint64_t dBytes[7] = {total + 64, total + 64, (n + 1) * 8, (n + 1) * 4, (n + 1) * sizeof(snapgpu_result_t),
                                3 * (n + 1) * sizeof(uint32_t), (n + 8) * SEEDS_PER_READ * sizeof(SeedRec)};
    // what the SAM / BAM calls take from the batch itself: the packed ids, the four per-record arrays
    // in one allocation, and (at most the last read's unclipped bases and qualities) the tail
    auto al16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t oIdLen = al16(n * 8), oFront = al16(oIdLen + n * 4), oFull = al16(oFront + n * 4),
                   metaBytes = al16(oFull + n * 4) + 16;
    need = idTotal + 16 + metaBytes + 2ull * hTot.maxBaseLen;
    for (uint64_t b : dBytes) need += b;
    if (int rc = fqFits(need, "the resident batch")) return rc;
    d = new snapgpu_device_reads_t();
    d->owner = a;
    d->n = n;
    d->device = a->device;
    d->hasIds = true;
    d->clipping = clipping;
    d->total = total;
    d->idTotal = idTotal;
    d->maxUnclipped = hTot.maxBaseLen;
    d->maxIdLen = hTot.maxIdLen;
    HIPCHK(hipMalloc(&d->dIds, idTotal + 16));
    HIPCHK(hipMalloc(&d->dMeta, metaBytes));
    d->dIdStart = (const uint64_t *)d->dMeta;
    d->dIdLen = (const uint32_t *)(d->dMeta + oIdLen);
    d->dFront = (const uint32_t *)(d->dMeta + oFront);
    d->dUnclipped = (const uint32_t *)(d->dMeta + oFull);
    HIPCHK(hipMemsetAsync(d->dIds + idTotal, 0, 16, s));
    HIPCHK(hipMalloc(&d->dBases, dBytes[0]));
    HIPCHK(hipMalloc(&d->dQuals, dBytes[1]));
    HIPCHK(hipMalloc(&d->dOffsets, dBytes[2]));
    HIPCHK(hipMalloc(&d->dLengths, dBytes[3]));
    HIPCHK(hipMalloc(&d->dOut, dBytes[4]));
    HIPCHK(hipMalloc(&d->dDefer, dBytes[5]));   // pass-1 / pass-2 defers, arena overflows
    HIPCHK(hipMalloc(&d->dSeeds, dBytes[6]));
    if (n) {
        HIPCHK(hipEventRecord(F.ev[7], s));
        fqgpu::pack(text, nBytes, (const uint64_t *)F.nl.p, nNl, n, R, (const uint64_t *)F.baseStart.p,
                    (const uint64_t *)F.idStart.p, d->dBases, d->dQuals, d->dIds, d->dOffsets, d->dLengths, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(F.ev[8], s));
        evUsed[2] = true;
        // the batch's own copies of what the next upload overwrites in the parser's buffers
        HIPCHK(hipMemcpyAsync(d->dMeta, F.idStart.p, n * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(d->dMeta + oIdLen, R.idLen, n * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(d->dMeta + oFront, R.front, n * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(d->dMeta + oFull, R.baseLen, n * 4, hipMemcpyDeviceToDevice, s));
        if (int rc = waitLane(a, a->lane[0])) return rc;
    }
    // 4. offsets and lengths always come back (the extent hash is a sequential chain); the batch on request
    t0 = clk::now();
    std::vector<uint64_t> tmpOff;
    std::vector<uint32_t> tmpLen;
    uint64_t *hOff;
    uint32_t *hLen;
    if (hostBatch) {
        r = snapgpu::allocReads(n, total, false, /*zero=*/false);
        r->ids = new char[idTotal + 1]();
        r->idOffsets = new uint64_t[n + 1]();
        r->idLengths = new uint32_t[n + 1]();
        if (clipping) {
            r->frontClipped = new uint32_t[n + 1]();
            r->unclippedLength = new uint32_t[n + 1]();
        }
        r->clipping = clipping;
        r->nUploads = 1;
        hOff = r->offsets;
        hLen = r->lengths;
        if (total) {
            HIPCHK(hipMemcpyAsync(r->bases, d->dBases, total, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipMemcpyAsync(r->quals, d->dQuals, total, hipMemcpyDeviceToHost, cs));
        }
        memset(r->bases + total, 0, 64);   // the batch's zero slack
        memset(r->quals + total, 0, 64);
        if (idTotal) HIPCHK(hipMemcpyAsync(r->ids, d->dIds, idTotal, hipMemcpyDeviceToHost, cs));
        if (n) {
            HIPCHK(hipMemcpyAsync(r->idOffsets, d->dIdStart, n * 8, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipMemcpyAsync(r->idLengths, d->dIdLen, n * 4, hipMemcpyDeviceToHost, cs));
            if (clipping) {
                HIPCHK(hipMemcpyAsync(r->frontClipped, d->dFront, n * 4, hipMemcpyDeviceToHost, cs));
                HIPCHK(hipMemcpyAsync(r->unclippedLength, d->dUnclipped, n * 4, hipMemcpyDeviceToHost, cs));
            }
        }
    } else {
        tmpOff.resize(n + 1);
        tmpLen.resize(n + 1);
        hOff = tmpOff.data();
        hLen = tmpLen.data();
    }
    if (n) {
        HIPCHK(hipMemcpyAsync(hOff, d->dOffsets, n * 8, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipMemcpyAsync(hLen, d->dLengths, n * 4, hipMemcpyDeviceToHost, cs));
    }
    HIPCHK(hipStreamSynchronize(cs));
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < n; i++) {   // as snapgpu_reads_upload
        const uint64_t endb = hOff[i] + hLen[i];
        if (endb > bytes) bytes = endb;
        if (hLen[i] > d->maxLen) d->maxLen = hLen[i];
        d->extentHash = extentMix(d->extentHash, hOff[i], hLen[i]);
    }
    if (bytes > total) { snapgpu::setError("fastq_upload: a clipped read ends past the batch"); return SNAPGPU_EDEVICE; }
    d->bytes = bytes;
    // the SAM / BAM lines print the unclipped SEQ and QUAL: what the zeroing takes stays in the tail
    if (const uint64_t tail = total - bytes) {
        if (tail > hTot.maxBaseLen) { snapgpu::setError("fastq_upload: the tail is longer than the longest read"); return SNAPGPU_EDEVICE; }
        HIPCHK(hipMalloc(&d->dTail, 2 * tail));
        HIPCHK(hipMemcpyAsync(d->dTail, d->dBases + bytes, tail, hipMemcpyDeviceToDevice, cs));
        HIPCHK(hipMemcpyAsync(d->dTail + tail, d->dQuals + bytes, tail, hipMemcpyDeviceToDevice, cs));
    }
    // zero from the largest clipped end on, as an upload of the clipped batch leaves it
    HIPCHK(hipMemsetAsync(d->dBases + bytes, 0, total + 64 - bytes, cs));
    HIPCHK(hipMemsetAsync(d->dQuals + bytes, 0, total + 64 - bytes, cs));
    HIPCHK(hipStreamSynchronize(cs));
    F.downloadMs = ms(t0);
    static const int kFirst[3] = {0, 3, 7}, kCount[3] = {2, 3, 1};   // the event groups and their intervals
    for (int k = 0, slot = 0; k < 3; slot += kCount[k], k++)
        if (evUsed[k])
            for (int j = 0; j < kCount[k]; j++) {
                float f = 0;
                HIPCHK(hipEventElapsedTime(&f, F.ev[kFirst[k] + j], F.ev[kFirst[k] + j + 1]));
                F.passMs[slot + j] = f;
                F.kernelMs += f;
            }
    F.kernelMs += F.arriveKernelMs;
    F.ran = true;
    return SNAPGPU_OK;
}

// the plain form's arrival: the text itself through the staging chunks
FastqArrival fastqPlainArrival(snapgpu_aligner_t *a, uint64_t nBytes, const FastqFill &fill) {
    FastqArrival A;
    A.nBytes = nBytes;
    A.arrive = [a, nBytes, &fill](char *text, uint64_t cap, char *last, double *) -> int {
        return fastqTextUpload(a, text, cap, nBytes, fill, last);
    };
    return A;
}

// The BGZF form's arrival: the compressed stream goes up and bgzf_inflate_kernel writes the text
// where the parser reads it; its last byte comes back.
FastqArrival fastqBgzfArrival(snapgpu_aligner_t *a, const char *in, uint64_t n, const std::vector<Member> &members,
                              uint64_t textBytes) {
    FastqArrival A;
    A.nBytes = textBytes;
    A.extraNeed = inflateGrowBytes(a, n, members.size());
    A.arrive = [a, in, n, &members, textBytes](char *text, uint64_t cap, char *last, double *kernelMs) -> int {
        HIPCHK(hipMemsetAsync(text + textBytes, 0, cap - textBytes, a->stream()));
        const int rc = inflateOnDevice(a, "fastq_upload_bgzf", in, n, members, text);
        *kernelMs = a->inf.kernelMs;
        if (rc) return rc;
        if (textBytes) HIPCHK(hipMemcpy(last, text + textBytes - 1, 1, hipMemcpyDeviceToHost));
        return (int)SNAPGPU_OK;
    };
    return A;
}

int fastqUpload(snapgpu_aligner_t *a, const FastqArrival &arrival, const char *name, int clipping,
                uint32_t flags, snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut) {
    if (dOut) *dOut = nullptr;
    if (readsOut) *readsOut = nullptr;
    const bool hostBatch = flags & SNAPGPU_FASTQ_HOST_BATCH;
    if (!a || !dOut || !name || (hostBatch && !readsOut) || clipping < 0 || clipping > 3 ||
        (flags & ~SNAPGPU_FASTQ_HOST_BATCH)) {
        snapgpu::setError("fastq_upload: bad argument");
        return SNAPGPU_EINVAL;
    }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    HIPCHK(hipSetDevice(a->device));
    snapgpu_device_reads_t *d = nullptr;
    snapgpu_reads_t *r = nullptr;
    const int rc = fastqRun(a, arrival, name, clipping, hostBatch, d, r);
    if (rc != SNAPGPU_OK) {
        snapgpu_device_reads_free(d);
        snapgpu_reads_free(r);
        return rc;
    }
    *dOut = d;
    if (hostBatch) *readsOut = r;
    return SNAPGPU_OK;
}

}  // namespace

void fastqStateFree(snapgpu_aligner_t *a) {
    auto &F = a->fq;
    auto &I = a->inf;
    for (DevBuf *b : {&F.text, &F.counts, &F.tileStart, &F.sums, &F.nl, &F.rec, &F.baseStart, &F.idStart, &F.sums2, &F.tot,
                      &I.in, &I.members, &I.status, &I.out})
        devFree(a, b->p);
    for (int k = 0; k < 2; k++) {
        if (!a->failed) hostPinnedFree(F.pin[k]);
        if (F.pinDone[k]) hipEventDestroy(F.pinDone[k]);
    }
    for (auto &e : F.ev) if (e) hipEventDestroy(e);
    for (auto &e : I.ev) if (e) hipEventDestroy(e);
}

extern "C" {

int snapgpu_fastq_upload(snapgpu_aligner_t *a, const char *text, uint64_t nBytes, const char *name, int clipping,
                         uint32_t flags, snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut) {
    if (!text && nBytes) {
        if (dOut) *dOut = nullptr;
        if (readsOut) *readsOut = nullptr;
        snapgpu::setError("fastq_upload: bad argument");
        return SNAPGPU_EINVAL;
    }
    const FastqFill fill = [text](char *dst, uint64_t off, uint64_t m) {
        fastqParallel(m, [=](uint64_t b, uint64_t e) { memcpy(dst + b, text + off + b, e - b); });
        return true;
    };
    return fastqUpload(a, fastqPlainArrival(a, nBytes, fill), name, clipping, flags, dOut, readsOut);
}

int snapgpu_fastq_upload_file(snapgpu_aligner_t *a, const char *path, int clipping, uint32_t flags,
                              snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut) {
    if (dOut) *dOut = nullptr;
    if (readsOut) *readsOut = nullptr;
    if (!path) { snapgpu::setError("fastq_upload: bad argument"); return SNAPGPU_EINVAL; }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { snapgpu::setError(std::string("cannot open ") + path); return SNAPGPU_EIO; }
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); snapgpu::setError(std::string("cannot stat ") + path); return SNAPGPU_EIO; }
    // the file goes straight into the staging chunks: one host pass over its bytes
    const FastqFill fill = [fd, path](char *dst, uint64_t off, uint64_t m) {
        std::atomic<bool> ok{true};
        fastqParallel(m, [&, dst, off](uint64_t b, uint64_t e) {
            while (b < e) {
                const ssize_t got = pread(fd, dst + b, e - b, (off_t)(off + b));
                if (got <= 0) { ok = false; return; }
                b += (uint64_t)got;
            }
        });
        if (!ok) snapgpu::setError(std::string("cannot read ") + path);
        return ok.load();
    };
    const int rc = fastqUpload(a, fastqPlainArrival(a, (uint64_t)sb.st_size, fill), path, clipping, flags, dOut, readsOut);
    close(fd);
    return rc;
}

int snapgpu_fastq_upload_bgzf(snapgpu_aligner_t *a, const char *data, uint64_t nBytes, const char *name, int clipping,
                              uint32_t flags, snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut) {
    if (dOut) *dOut = nullptr;
    if (readsOut) *readsOut = nullptr;
    if (!a || (!data && nBytes) || !name) {
        snapgpu::setError("fastq_upload_bgzf: bad argument");
        return SNAPGPU_EINVAL;
    }
    std::vector<Member> members;
    uint64_t textBytes = 0;
    if (int rc = snapgpu::bgzfWalk("fastq_upload_bgzf", data, nBytes, members, &textBytes)) return rc;
    return fastqUpload(a, fastqBgzfArrival(a, data, nBytes, members, textBytes), name, clipping, flags, dOut, readsOut);
}

int snapgpu_fastq_upload_bgzf_file(snapgpu_aligner_t *a, const char *path, int clipping, uint32_t flags,
                                   snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut) {
    if (dOut) *dOut = nullptr;
    if (readsOut) *readsOut = nullptr;
    if (!path) { snapgpu::setError("fastq_upload_bgzf: bad argument"); return SNAPGPU_EINVAL; }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { snapgpu::setError(std::string("cannot open ") + path); return SNAPGPU_EIO; }
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); snapgpu::setError(std::string("cannot stat ") + path); return SNAPGPU_EIO; }
    // the member walk hops through the whole stream, so the compressed file is read first
    const uint64_t size = (uint64_t)sb.st_size;
    std::unique_ptr<char[]> data(new char[size ? size : 1]);
    std::atomic<bool> ok{true};
    char *dst = data.get();
    fastqParallel(size, [&ok, fd, dst](uint64_t b, uint64_t e) {
        while (b < e) {
            const ssize_t got = pread(fd, dst + b, e - b, (off_t)b);
            if (got <= 0) { ok = false; return; }
            b += (uint64_t)got;
        }
    });
    close(fd);
    if (!ok) { snapgpu::setError(std::string("cannot read ") + path); return SNAPGPU_EIO; }
    return snapgpu_fastq_upload_bgzf(a, data.get(), size, path, clipping, flags, dOut, readsOut);
}

int snapgpu_bgzf_inflate_gpu(snapgpu_aligner_t *a, const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used) {
    if (!a || (!in && n) || !used) { snapgpu::setError("bgzf_inflate_gpu: null argument"); return SNAPGPU_EINVAL; }
    *used = 0;
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    std::vector<Member> members;
    uint64_t total = 0;
    if (int rc = snapgpu::bgzfWalk("bgzf_inflate_gpu", in, n, members, &total)) return rc;
    *used = total;
    if (total > cap || (!out && total)) { snapgpu::setError("bgzf_inflate_gpu: output buffer too small"); return SNAPGPU_EINVAL; }
    HIPCHK(hipSetDevice(a->device));
    auto &I = a->inf;
    if (int rc = fqFits(inflateGrowBytes(a, n, members.size()) + growBytes(I.out, total + 64), "the stream and its output")) return rc;
    HIPCHK(devGrow(a, I.out, total + 64));
    if (int rc = inflateOnDevice(a, "bgzf_inflate_gpu", in, n, members, (char *)I.out.p)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (total)
        if (int rc = textDownload(a, (const char *)I.out.p, total, out)) return rc;
    I.downloadMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SNAPGPU_OK;
}

int snapgpu_bgzf_inflate_last_ms(snapgpu_aligner_t *a, double *uploadMs, double *kernelMs, double *downloadMs) {
    if (!a || !uploadMs || !kernelMs || !downloadMs) return SNAPGPU_EINVAL;
    if (!a->inf.ran) { snapgpu::setError("bgzf_inflate_last_ms: no device inflate on this aligner"); return SNAPGPU_EINVAL; }
    *uploadMs = a->inf.uploadMs;
    *kernelMs = a->inf.kernelMs;
    *downloadMs = a->inf.downloadMs;
    return SNAPGPU_OK;
}

int snapgpu_bgzf_inflate_waves(snapgpu_aligner_t *a) {
    if (!a) { snapgpu::setError("bgzf_inflate_waves: null argument"); return SNAPGPU_EINVAL; }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    if (int rc = inflateWaves(a)) return rc;
    return a->inf.waves;
}

int snapgpu_fastq_last_ms(snapgpu_aligner_t *a, double *uploadMs, double *kernelMs, double *downloadMs) {
    if (!a || !uploadMs || !kernelMs || !downloadMs) return SNAPGPU_EINVAL;
    if (!a->fq.ran) { snapgpu::setError("fastq_last_ms: no device FASTQ parse on this aligner"); return SNAPGPU_EINVAL; }
    *uploadMs = a->fq.uploadMs;
    *kernelMs = a->fq.kernelMs;
    *downloadMs = a->fq.downloadMs;
    return SNAPGPU_OK;
}

uint32_t snapgpu_fastq_tile_bytes(void) { return fqgpu::kTileBytes; }

// ms[0 .. 6): newline count, its scan, line starts, record pass, the two length scans, copy pass of the
// last device FASTQ parse (tools/fastq_parse_time.py)
int snapgpu_internal_fastq_pass_ms(snapgpu_aligner_t *a, double *ms) {
    if (!a || !ms || !a->fq.ran) return SNAPGPU_EINVAL;
    for (int k = 0; k < 6; k++) ms[k] = a->fq.passMs[k];
    return SNAPGPU_OK;
}

int snapgpu_device_reads_peek(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint64_t *n, uint64_t *bytes,
                              uint32_t *maxLen, uint64_t *extentHash, uint64_t *offsets, uint32_t *lengths,
                              char *bases, char *quals) {
    if (!a || !d || d->owner != a) { snapgpu::setError("device_reads_peek: bad argument"); return SNAPGPU_EINVAL; }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    HIPCHK(hipSetDevice(a->device));
    if (n) *n = d->n;
    if (bytes) *bytes = d->bytes;
    if (maxLen) *maxLen = d->maxLen;
    if (extentHash) *extentHash = d->extentHash;
    if (offsets && d->n) HIPCHK(hipMemcpy(offsets, d->dOffsets, d->n * 8, hipMemcpyDeviceToHost));
    if (lengths && d->n) HIPCHK(hipMemcpy(lengths, d->dLengths, d->n * 4, hipMemcpyDeviceToHost));
    if (bases) HIPCHK(hipMemcpy(bases, d->dBases, d->bytes + 64, hipMemcpyDeviceToHost));
    if (quals) HIPCHK(hipMemcpy(quals, d->dQuals, d->bytes + 64, hipMemcpyDeviceToHost));
    return SNAPGPU_OK;
}

int snapgpu_device_reads_ids_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *ids, uint64_t cap,
                                      uint64_t *used, uint64_t *idOffsets, uint32_t *idLengths, uint32_t *frontClipped,
                                      uint32_t *unclippedLength) {
    if (!a || !d || !used || d->owner != a) { snapgpu::setError("device_reads_ids_download: bad argument"); return SNAPGPU_EINVAL; }
    *used = 0;
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    if (!d->hasIds) {
        snapgpu::setError("device_reads_ids_download: the resident batch holds no ids of its own (only snapgpu_fastq_upload leaves them)");
        return SNAPGPU_EINVAL;
    }
    *used = d->idTotal;
    if (d->idTotal > cap || (!ids && d->idTotal)) {
        snapgpu::setError("device_reads_ids_download: output buffer too small");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    if (d->idTotal) HIPCHK(hipMemcpy(ids, d->dIds, d->idTotal, hipMemcpyDeviceToHost));
    if (d->n) {
        if (idOffsets) HIPCHK(hipMemcpy(idOffsets, d->dIdStart, d->n * 8, hipMemcpyDeviceToHost));
        if (idLengths) HIPCHK(hipMemcpy(idLengths, d->dIdLen, d->n * 4, hipMemcpyDeviceToHost));
        if (d->clipping) {
            if (frontClipped) HIPCHK(hipMemcpy(frontClipped, d->dFront, d->n * 4, hipMemcpyDeviceToHost));
            if (unclippedLength) HIPCHK(hipMemcpy(unclippedLength, d->dUnclipped, d->n * 4, hipMemcpyDeviceToHost));
        }
    }
    return SNAPGPU_OK;
}

}  // extern "C"
