// output_chain.hip -- the host side of the resident output chain behind include/snapgpu.h: SAM text
// (sam_format.hip), BAM records (bam_format.hip), duplicate marking (dupmark.hip), BGZF (bgzf.hip) and
// the BAI index (bai.hip), each over a resident batch and in a batch form.  No kernels here: the
// stages' launches, their ordering on the aligner's streams, the downloads and the entry points.
// The state types, and what a stage gets from StageState, are in aligner_state.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "aligner_state.h"
#include "bam_format.h"
#include "bgzf.h"

void stageFree(const snapgpu_aligner_t *a, StageState &S) {
    for (DevBuf *b : S.bufs) {
        devFree(a, b->p);
        b->p = nullptr;
        b->cap = 0;
    }
    if (!(a && a->failed))
        for (auto &e : S.ev)
            if (e) { hipEventDestroy(e); e = nullptr; }
}

int stageEvents(StageState &S) {
    for (int k = 0; k < S.nEv; k++)
        if (!S.ev[k]) HIPCHK(hipEventCreate(&S.ev[k]));
    return SNAPGPU_OK;
}

// What most entry points begin with: 0, or the code to return (the message is set).  argsOk: no
// other argument is missing; d: a resident batch that has to be this aligner's.
static int enter(const char *name, const snapgpu_aligner_t *a, bool argsOk, const snapgpu_device_reads_t *d = nullptr) {
    if (!a || !argsOk) { snapgpu::setError(std::string(name) + ": null argument"); return SNAPGPU_EINVAL; }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    if (d && d->owner != a) { snapgpu::setError(std::string(name) + ": the resident batch belongs to another aligner"); return SNAPGPU_EINVAL; }
    return SNAPGPU_OK;
}

// *S = the state stage st's last call used (needRan: and still current), for the calls that report
// its times; `none`: the message when there is none.
static int lastStage(snapgpu_aligner_t *a, Stage st, bool needRan, const char *none, StageState **S) {
    *S = a->last[st];
    if (!*S || (needRan && !(*S)->ran)) { snapgpu::setError(none); return SNAPGPU_EINVAL; }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    HIPCHK(hipSetDevice(a->device));
    return SNAPGPU_OK;
}

// The *_last_ms calls: the kernels' ms between events `from` and `to` of stage st's last call (0 when
// it had nothing to run) and its download's wall ms.
static int stageLastMs(snapgpu_aligner_t *a, Stage st, bool needRan, const char *none, int from, int to, double *kernelMs,
                       double *downloadMs) {
    if (!a || !kernelMs || !downloadMs) return SNAPGPU_EINVAL;
    StageState *S;
    if (int rc = lastStage(a, st, needRan, none, &S)) return rc;
    float f = 0;
    if (!S->empty) {
        HIPCHK(hipEventSynchronize(S->ev[to]));
        HIPCHK(hipEventElapsedTime(&f, S->ev[from], S->ev[to]));
    }
    *kernelMs = f;
    *downloadMs = S->downloadMs;
    return SNAPGPU_OK;
}

// The snapgpu_internal_*_pass_ms calls: ms[k] = the kernels between events k and k + 1 of stage st's
// last call, for all its events.
static int stagePassMs(snapgpu_aligner_t *a, Stage st, bool needRan, double *ms) {
    StageState *S = a && ms && !a->failed ? a->last[st] : nullptr;
    if (!S || (needRan && !S->ran)) return SNAPGPU_EINVAL;
    HIPCHK(hipSetDevice(a->device));
    for (int k = 0; k + 1 < S->nEv; k++) {
        float f = 0;
        if (!S->empty) {
            HIPCHK(hipEventSynchronize(S->ev[k + 1]));
            HIPCHK(hipEventElapsedTime(&f, S->ev[k], S->ev[k + 1]));
        }
        ms[k] = f;
    }
    return SNAPGPU_OK;
}

// ------------------------------------------------- SAM text on the device (sam_format.hip)
static const uint64_t kSamChunk = 16ull << 20;   // bytes per pinned staging chunk of the text download

// The small host-side inputs of the formatter, packed for one upload.
struct SamHostIn {
    uint64_t n = 0;
    const uint64_t *offsets = nullptr;   // null: already on the device (resident batch)
    const uint32_t *lengths = nullptr;
    const char *ids = nullptr;
    const uint64_t *idOffsets = nullptr;
    const uint32_t *idLengths = nullptr;
    const uint32_t *front = nullptr, *unclipped = nullptr;
    const char *rg = nullptr;
    // the device form (a resident batch's own state, no host batch): what is set here is already in
    // device memory and is pointed at, not uploaded
    const char *dIds = nullptr;            // with dIdOffsets / dIdLengths, when ids is null
    const uint64_t *dIdOffsets = nullptr;
    const uint32_t *dIdLengths = nullptr;
    const uint32_t *dFront = nullptr, *dUnclipped = nullptr;
    bool device = false;                   // lengths is null: the bound comes from the totals below
    uint64_t idTotal = 0, baseTotal = 0;   // bytes of all ids (the caller's, if it passed ids), of all unclipped reads
};

// Upload H's arrays, the piece names and the read group into S.aux (unless S still holds them:
// skip) and point A at them; textBound = a bound on the bytes of text from the host's side.
static int samPrepare(snapgpu_aligner_t *a, SamState &S, const SamHostIn &H, bool skip, samline::Args &A) {
    const uint64_t n = H.n;
    const snapgpu::Genome &g = *a->idx->genome;
    std::vector<uint32_t> nameOff;
    std::string names;
    snapgpu::samPieceNames(g, nameOff, names);
    std::vector<uint32_t> sortBase;
    std::vector<uint8_t> sortNone;
    snapgpu::samSortBases(g, sortBase, sortNone);
    const uint32_t rgLen = H.rg ? (uint32_t)strlen(H.rg) : 0u;
    uint64_t idBytes = 0, bound = 0;
    uint32_t maxName = 1;
    for (size_t p = 0; p + 1 < nameOff.size(); p++) maxName = std::max(maxName, nameOff[p + 1] - nameOff[p]);
    // per line: flags, POS, MAPQ, tabs, mate fields, tags and NM (< 64), RNAME, two soft clips and
    // SNAPGPU_CIGAR_MAX_OPS ops of at most 11 bytes each
    const uint64_t perLine = 64 + maxName + (H.rg ? 6 + rgLen : 0) + 22 + 11ull * SNAPGPU_CIGAR_MAX_OPS;
    if (H.ids)
        for (uint64_t i = 0; i < n; i++) idBytes = std::max<uint64_t>(idBytes, H.idOffsets[i] + H.idLengths[i]);
    if (H.device) {
        bound = H.idTotal + 2 * H.baseTotal + n * perLine;
    } else {
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t len = H.unclipped ? H.unclipped[i] : H.lengths[i];
            bound += H.idLengths[i] + 2ull * std::min(len, samline::kMaxSeq) + perLine;
        }
    }
    S.textBound = bound;
    AuxPack P;
    const uint64_t nIds = H.ids ? n : 0;   // the id arrays ride in aux only when they come from the host
    const uint64_t nClip = H.unclipped ? n : 0, nExt = H.offsets ? n : 0;
    const uint64_t oIdOff = P.add(H.idOffsets, nIds * 8), oIdLen = P.add(H.idLengths, nIds * 4),
                   oFront = P.add(H.front, nClip * 4), oFull = P.add(H.unclipped, nClip * 4),
                   oOff = P.add(H.offsets, nExt * 8), oLen = P.add(H.lengths, nExt * 4),
                   oNameOff = P.add(nameOff.data(), nameOff.size() * 4), oNames = P.add(names.data(), names.size()),
                   oSortBase = P.add(sortBase.data(), sortBase.size() * 4), oSortNone = P.add(sortNone.data(), sortNone.size()),
                   oRg = P.add(H.rg, rgLen), oIds = P.add(H.ids, idBytes);
    if (!skip) {
        if (S.ran && S.ev[1]) HIPCHK(hipEventSynchronize(S.ev[1]));   // an earlier call's kernels may still read aux
        HIPCHK(devGrow(a, S.aux, P.bytes()));
        P.copyTo(S.hAux);
        // on the otherwise idle copy stream, and waited for: the host copy may go, and the side
        // stream (which may still be in the CIGAR kernel) is not waited for
        HIPCHK(hipMemcpyAsync(S.aux.p, S.hAux.data(), P.bytes(), hipMemcpyHostToDevice, a->copyStream));
        HIPCHK(hipStreamSynchronize(a->copyStream));
    }
    const char *d = (const char *)S.aux.p;
    A.idOffsets = H.ids ? (const uint64_t *)(d + oIdOff) : H.dIdOffsets;
    A.idLengths = H.ids ? (const uint32_t *)(d + oIdLen) : H.dIdLengths;
    A.front = H.unclipped ? (const uint32_t *)(d + oFront) : H.dFront;
    A.unclipped = H.unclipped ? (const uint32_t *)(d + oFull) : H.dUnclipped;
    if (H.offsets) { A.offsets = (const uint64_t *)(d + oOff); A.lengths = (const uint32_t *)(d + oLen); }
    A.pieceOffsets = a->dPieces;
    A.pieceNameOff = (const uint32_t *)(d + oNameOff);
    A.pieceNames = d + oNames;
    S.sortArgs = samline::SortArgs{(const uint32_t *)(d + oSortBase), (const uint8_t *)(d + oSortNone)};
    A.nPieces = (int32_t)g.pieceOffsets.size();
    A.rg = H.rg ? d + oRg : nullptr;
    A.rgLen = rgLen;
    A.ids = H.ids ? d + oIds : H.dIds;
    return SNAPGPU_OK;
}

// The sort step's buffers of a sorted call over n records: S's, grown, into SB.
int sortBuffers(snapgpu_aligner_t *a, SamState &S, uint64_t n, samgpu::SortBuffers *SB) {
    HIPCHK(samgpu::sortTempBytes(n, a->sideStream, &SB->tempBytes));
    for (DevBuf *b : {&S.key, &S.keySorted, &S.iota, &S.order, &S.slotLen}) HIPCHK(devGrow(a, *b, n * 4));
    HIPCHK(devGrow(a, S.sortTemp, SB->tempBytes));
    SB->key = (uint32_t *)S.key.p; SB->keySorted = (uint32_t *)S.keySorted.p;
    SB->iota = (uint32_t *)S.iota.p; SB->order = (uint32_t *)S.order.p;
    SB->slotLen = (uint32_t *)S.slotLen.p;
    SB->temp = S.sortTemp.p;
    return SNAPGPU_OK;
}

int textBuffers(const snapgpu_aligner_t *a, SamState &S, uint64_t n, samgpu::Buffers *B) {
    if (n > 0xffffffffull) { snapgpu::setError("batch too large"); return SNAPGPU_EINVAL; }
    HIPCHK(devGrow(a, S.len, n * 4));
    HIPCHK(devGrow(a, S.scans, n * sizeof(samline::Scans)));
    HIPCHK(devGrow(a, S.start, (n + 1) * 8));
    HIPCHK(devGrow(a, S.sums, samgpu::scanTiles(n) * 8));
    HIPCHK(devGrow(a, S.bad, 16));
    HIPCHK(devGrow(a, S.text, S.textBound + 16));
    *B = samgpu::Buffers{(uint32_t *)S.len.p, (samline::Scans *)S.scans.p, (uint64_t *)S.start.p, (uint64_t *)S.sums.p,
                         (char *)S.text.p, S.textBound, (uint32_t *)S.bad.p, {nullptr, nullptr}};
    return SNAPGPU_OK;
}

// Length pass, scan, write pass and check of n records on the side stream, into S's buffers;
// sorted: in the stable order of the records' coordinate-sort keys (S.order keeps that order).
static int samLaunch(snapgpu_aligner_t *a, SamState &S, const samline::Args &A, uint64_t n, bool sorted) {
    if (int rc = stageEvents(S)) return rc;
    S.n = n;
    S.empty = n == 0;
    S.ran = true;
    S.sorted = sorted;
    a->last[kStageSam] = &S;
    if (n == 0) return SNAPGPU_OK;
    samgpu::Buffers B;
    if (int rc = textBuffers(a, S, n, &B)) return rc;
    B.mid[0] = S.ev[2];
    B.mid[1] = S.ev[3];
    samgpu::SortBuffers SB{};
    if (sorted) {
        if (int rc = sortBuffers(a, S, n, &SB)) return rc;
        SB.keys = S.sortArgs;
        SB.done = S.ev[4];
    }
    HIPCHK(hipEventRecord(S.ev[0], a->sideStream));
    HIPCHK(samgpu::launch(A, n, B, a->sideStream, sorted ? &SB : nullptr));
    HIPCHK(hipEventRecord(S.ev[1], a->sideStream));
    return SNAPGPU_OK;
}

int textDownload(snapgpu_aligner_t *a, const char *text, uint64_t total, char *out) {
    for (int k = 0; k < 2; k++) {
        if (!a->samPin[k]) HIPCHK(hipHostMalloc(&a->samPin[k], kSamChunk, hipHostMallocDefault));
        if (!a->samPinDone[k]) HIPCHK(hipEventCreateWithFlags(&a->samPinDone[k], hipEventDisableTiming));
    }
    const uint64_t nChunks = (total + kSamChunk - 1) / kSamChunk;
    auto issue = [&](uint64_t k) -> hipError_t {
        const uint64_t b = k * kSamChunk, m = std::min(kSamChunk, total - b);
        hipError_t e = hipMemcpyAsync(a->samPin[k & 1], text + b, m, hipMemcpyDeviceToHost, a->sideStream);
        return e != hipSuccess ? e : hipEventRecord(a->samPinDone[k & 1], a->sideStream);
    };
    const unsigned nt = snapgpu::hostThreads(16);
    HIPCHK(issue(0));
    for (uint64_t k = 0; k < nChunks; k++) {
        if (k + 1 < nChunks) HIPCHK(issue(k + 1));
        if (int rc = waitEvent(a, a->samPinDone[k & 1])) return rc;
        const uint64_t b = k * kSamChunk, m = std::min(kSamChunk, total - b);
        const char *src = (const char *)a->samPin[k & 1];
        const unsigned t = m < (1u << 20) ? 1u : nt;
        std::vector<std::thread> th;
        for (unsigned j = 1; j < t; j++)
            th.emplace_back([=] { memcpy(out + b + m * j / t, src + m * j / t, m * (j + 1) / t - m * j / t); });
        memcpy(out + b, src, m / t);
        for (auto &x : th) x.join();
    }
    return SNAPGPU_OK;
}

int textFinish(snapgpu_aligner_t *a, SamState &S, const StageWords &W, char *out, uint64_t cap, uint64_t *used,
               int (*checked)(SamState &, void *), void *arg) {
    *used = 0;
    S.downloadMs = 0;
    if (S.n == 0) return SNAPGPU_OK;
    if (int rc = waitEvent(a, S.ev[1])) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t total = 0;
    uint32_t bad = 0;
    HIPCHK(hipMemcpy(&total, (const uint64_t *)S.start.p + S.n, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&bad, S.bad.p, 4, hipMemcpyDeviceToHost));
    if (bad || total > S.textBound) {
        char msg[160];
        snprintf(msg, sizeof msg, W.checkFmt, bad, (unsigned long long)S.n, (unsigned long long)total,
                 (unsigned long long)S.textBound);
        snapgpu::setError(msg);
        return SNAPGPU_EDEVICE;
    }
    if (checked)
        if (int rc = checked(S, arg)) return rc;
    *used = total;
    if (total > cap || !out) { snapgpu::setError(std::string(W.call) + ": output buffer too small"); return SNAPGPU_EINVAL; }
    if (int rc = textDownload(a, (const char *)S.text.p, total, out)) return rc;
    S.downloadMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SNAPGPU_OK;
}

static int samDownload(snapgpu_aligner_t *a, SamState &S, char *out, uint64_t cap, uint64_t *used) {
    return textFinish(a, S, {"sam: %u of %llu lines do not end where the scan placed them (text %llu bytes, bound %llu)", "sam_download"},
                      out, cap, used);
}

// The device BAM encoder's passes over n records on the side stream, into S's buffers (samLaunch's
// counterpart; S.textBound is samPrepare's bound on the SAM text, which exceeds the records' bytes:
// per record the id, 1.5 bytes per base and at most 36 + 1 + 4 * 66 + 4 + 15 more, plus the read group).
static int bamLaunch(snapgpu_aligner_t *a, BamState &S, const samline::Args &A, uint64_t n, bool sorted, int32_t nmCarryIn) {
    if (int rc = stageEvents(S)) return rc;
    S.n = n;
    S.empty = n == 0;
    S.ran = true;
    S.sorted = sorted;
    S.carryIn = nmCarryIn;
    a->last[kStageBam] = &S;
    if (n == 0) return SNAPGPU_OK;
    if (n > 0xffffffffull) { snapgpu::setError("batch too large"); return SNAPGPU_EINVAL; }
    HIPCHK(devGrow(a, S.len, n * 4));
    HIPCHK(devGrow(a, S.nm, n * 4));
    HIPCHK(devGrow(a, S.nmTiles, samgpu::scanTiles(n) * 4));
    HIPCHK(devGrow(a, S.start, (n + 1) * 8));
    HIPCHK(devGrow(a, S.sums, samgpu::scanTiles(n) * 8));
    HIPCHK(devGrow(a, S.bad, 16));
    HIPCHK(devGrow(a, S.text, S.textBound + 16));
    const bamgpu::Buffers B{(uint32_t *)S.len.p, (int32_t *)S.nm.p, (int32_t *)S.nmTiles.p, (uint64_t *)S.start.p,
                            (uint64_t *)S.sums.p, (char *)S.text.p, S.textBound, (uint32_t *)S.bad.p};
    samgpu::SortBuffers SB{};
    if (sorted)
        if (int rc = sortBuffers(a, S, n, &SB)) return rc;
    HIPCHK(hipEventRecord(S.ev[0], a->sideStream));
    HIPCHK(bamgpu::launch(A, n, nmCarryIn, B, a->sideStream, sorted ? &SB : nullptr));
    HIPCHK(hipEventRecord(S.ev[1], a->sideStream));
    return SNAPGPU_OK;
}

// textFinish over the records, and the carry-out: the carry-in again unless the check passed.
static int bamDownload(snapgpu_aligner_t *a, BamState &S, char *out, uint64_t cap, uint64_t *used, int32_t *nmCarryOut) {
    if (nmCarryOut) *nmCarryOut = S.carryIn;
    auto carryOut = [](SamState &B, void *to) -> int {
        if (to) HIPCHK(hipMemcpy(to, (const int32_t *)static_cast<BamState &>(B).nm.p + B.n - 1, 4, hipMemcpyDeviceToHost));
        return SNAPGPU_OK;
    };
    return textFinish(a, S, {"bam: %u of %llu records do not carry the size the scan gave them (output %llu bytes, bound %llu)", "bam_download"},
                      out, cap, used, carryOut, nmCarryOut);
}

// Wait for the mark passes of S and take their counts; SNAPGPU_EDEVICE unless they add up.
static int dupResult(snapgpu_aligner_t *a, DupState &S, dupgpu::Result *r) {
    if (int rc = waitEvent(a, S.ev[dupgpu::kPasses])) return rc;
    HIPCHK(hipMemcpy(r, (const char *)S.work.p + S.L.res, sizeof *r, hipMemcpyDeviceToHost));
    if (r->refused || r->mates || r->marked != r->expected) {
        char msg[240];
        snprintf(msg, sizeof msg, "dupmark: %u records are refused or out of (refID, pos) order, %u carry a mate (FLAG 0x1), "
                                  "%llu records marked where the groups' sizes give %llu",
                 r->refused, r->mates, r->marked, r->expected);
        snapgpu::setError(msg);
        return SNAPGPU_EDEVICE;
    }
    return SNAPGPU_OK;
}

// snapgpu_sam_resident and snapgpu_sam_resident_sorted; bam: snapgpu_bam_resident and
// snapgpu_bam_resident_sorted, the same checks and ordering over the batch's BAM state
static int samResident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                       const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                       const char *readGroup, bool sorted, bool bam = false, int32_t nmCarryIn = 0) {
    const std::string who = bam ? "bam_resident" : "sam_resident";
    if (int rc = enter(who.c_str(), a, d != nullptr, d)) return rc;
    // reads == NULL: the batch's own resident ids and clip state (the device FASTQ parser's), nothing
    // to compare the extents with
    const bool devForm = !reads;
    const uint64_t n = d->n;
    if (devForm && !d->hasIds) {
        snapgpu::setError(who + ": reads is NULL and the resident batch holds no ids or clip state of its own "
                                "(only snapgpu_fastq_upload leaves them; pass the batch it was uploaded from)");
        return SNAPGPU_EINVAL;
    }
    if (!devForm) {
        uint64_t bytes = 0, hash = 0;
        if (reads->n == d->n)
            for (uint64_t i = 0; i < reads->n; i++) {
                bytes = std::max<uint64_t>(bytes, reads->offsets[i] + reads->lengths[i]);
                hash = extentMix(hash, reads->offsets[i], reads->lengths[i]);
            }
        if (reads->n != d->n || bytes != d->bytes || hash != d->extentHash) {
            snapgpu::setError(who + ": the reads batch does not match the resident batch (n, offsets or lengths differ)");
            return SNAPGPU_EINVAL;
        }
    }
    const bool ownIds = !ids;
    if (ownIds && !devForm) { ids = reads->ids; idOffsets = reads->idOffsets; idLengths = reads->idLengths; }
    if (!(ownIds && devForm) && (!ids || !idOffsets || !idLengths)) {
        snapgpu::setError(who + ": no read ids (pass ids, or use a batch that carries them)");
        return SNAPGPU_EINVAL;
    }
    const uint32_t *front = nullptr, *unclipped = nullptr;
    if (devForm) {
        // the host loops' verdicts from the maxima the upload fetched, with their messages
        const uint32_t one[1] = {ownIds ? d->maxIdLen : 0u};
        if (bam)
            if (int rc = ownIds ? snapgpu::bamCheckIds(one, 1) : snapgpu::bamCheckIds(idLengths, n)) return rc;
        if (d->maxUnclipped > 1024) {
            snapgpu::setError("sam_format: nOps > SNAPGPU_CIGAR_MAX_OPS, read longer than 1024 bases or bad clip arrays");
            return SNAPGPU_EINVAL;
        }
    } else {
        if (bam)
            if (int rc = snapgpu::bamCheckIds(idLengths, n)) return rc;
        if (int rc = snapgpu::samCheckClips(reads, nullptr, &front, &unclipped)) return rc;
    }
    if (!d->dCigEd) {
        snapgpu::setError(who + ": no snapgpu_cigar_resident before snapgpu_" + who);
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    SamState &S = bam ? d->bam : d->sam;
    hipStream_t st = a->sideStream;
    // snapgpu_reads_upload copied bases and qualities up to the largest clipped end: where the
    // unclipped extents (SEQ / QUAL) pass it, the formatter reads a copy that holds them all
    uint64_t need = d->bytes;
    if (devForm && d->dTail) need = d->total;   // the last read's unclipped end
    if (unclipped)
        for (uint64_t i = 0; i < reads->n; i++)
            need = std::max<uint64_t>(need, reads->offsets[i] - front[i] + unclipped[i]);
    if (need > d->bytes && S.fullBytes != need) {
        if (S.ran && S.ev[1]) HIPCHK(hipEventSynchronize(S.ev[1]));
        const uint64_t tail = need - d->bytes;
        if (!devForm) {
            S.hAux.assign(2 * tail, 0);
            memcpy(S.hAux.data(), reads->bases + d->bytes, tail);
            memcpy(S.hAux.data() + tail, reads->quals + d->bytes, tail);
        }
        for (int q = 0; q < 2; q++) {
            DevBuf &b = q ? S.quals : S.bases;
            HIPCHK(devGrow(a, b, need + 64));
            HIPCHK(hipMemsetAsync((char *)b.p + need, 0, 64, a->copyStream));
            HIPCHK(hipMemcpyAsync(b.p, q ? d->dQuals : d->dBases, d->bytes, hipMemcpyDeviceToDevice, a->copyStream));
            if (devForm)   // the resident tail: no host bytes
                HIPCHK(hipMemcpyAsync((char *)b.p + d->bytes, d->dTail + q * tail, tail, hipMemcpyDeviceToDevice, a->copyStream));
            else
                HIPCHK(hipMemcpyAsync((char *)b.p + d->bytes, S.hAux.data() + q * tail, tail, hipMemcpyHostToDevice, a->copyStream));
        }
        HIPCHK(hipStreamSynchronize(a->copyStream));
        S.fullBytes = need;
    }
    samline::Args A;
    memset(&A, 0, sizeof(A));
    const bool full = need > d->bytes;
    A.bases = full ? (const char *)S.bases.p : d->dBases;
    A.quals = full ? (const char *)S.quals.p : d->dQuals;
    A.offsets = d->dOffsets;
    A.lengths = d->dLengths;
    A.res = d->dOut;
    A.ed = d->dCigEd;
    A.nOps = d->dCigN;
    A.ops = d->dCigOps;
    SamHostIn H;
    H.n = n;
    H.ids = ids; H.idOffsets = idOffsets; H.idLengths = idLengths;
    H.rg = readGroup;
    if (devForm) {
        // aux carries only the piece names, the sort bases and the read group (and a caller's ids)
        H.device = true;
        H.baseTotal = d->total;
        H.idTotal = d->idTotal;
        if (ownIds) {
            H.dIds = d->dIds; H.dIdOffsets = d->dIdStart; H.dIdLengths = d->dIdLen;
        } else {
            H.idTotal = 0;
            for (uint64_t i = 0; i < n; i++) H.idTotal += idLengths[i];
        }
        if (d->clipping) { H.dFront = d->dFront; H.dUnclipped = d->dUnclipped; }
    } else {
        H.lengths = reads->lengths;   // offsets and lengths are resident: the lengths only bound the text
        H.front = front; H.unclipped = unclipped;
    }
    // the batch's own ids do not change: their upload (or, in the device form, the upload without them)
    // is kept for the next call of the same form with the same read group
    const bool skip = ownIds && S.idsCached && S.cachedDevForm == devForm && S.cachedHasRg == (readGroup != nullptr) &&
                      (!readGroup || S.cachedRg == readGroup);
    if (int rc = samPrepare(a, S, H, skip, A)) return rc;
    S.idsCached = ownIds;
    S.cachedDevForm = devForm;
    S.cachedHasRg = readGroup != nullptr;
    S.cachedRg = readGroup ? readGroup : "";
    // the records may come from pass sets on both lanes; the CIGAR kernel is ahead on this stream
    for (auto &L : a->lane) {
        HIPCHK(hipEventRecord(L.done, L.stream));
        HIPCHK(hipStreamWaitEvent(st, L.done, 0));
    }
    // the records change: a compressed stream of the earlier ones, its index and their marking are stale
    if (bam) d->bgzf.ran = d->bai.ran = d->dup.ran = false;
    if (int rc = bam ? bamLaunch(a, d->bam, A, n, sorted, nmCarryIn) : samLaunch(a, S, A, n, sorted)) return rc;
    // the next pass set over these reads rewrites the records: it waits for the SAM / BAM kernels
    HIPCHK(hipEventRecord(a->residentSideDone, st));
    a->residentSidePending = true;
    return SNAPGPU_OK;
}

// Wait for S's kernels and copy the output order of its last (sorted) call to the host.
static int samOrderDownload(snapgpu_aligner_t *a, SamState &S, uint32_t *order) {
    if (S.n == 0) return SNAPGPU_OK;
    if (int rc = waitEvent(a, S.ev[1])) return rc;
    HIPCHK(hipMemcpy(order, S.order.p, S.n * 4, hipMemcpyDeviceToHost));
    return SNAPGPU_OK;
}

// snapgpu_sam_order_download and snapgpu_bam_order_download over the batch's state S of that stage
// (null with d); notSorted: the message when its last call left no order
static int orderDownload(const char *who, const char *notSorted, snapgpu_aligner_t *a, SamState *S, uint32_t *order) {
    if (int rc = enter(who, a, S != nullptr)) return rc;
    if (!S->ran || !S->sorted) { snapgpu::setError(notSorted); return SNAPGPU_EINVAL; }
    if (!order && S->n) { snapgpu::setError(std::string(who) + ": null argument"); return SNAPGPU_EINVAL; }
    HIPCHK(hipSetDevice(a->device));
    return samOrderDownload(a, *S, order);
}

// snapgpu_sam_format_gpu and snapgpu_sam_format_gpu_sorted (order: the output order, or null)
static int samFormatBatch(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                          const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                          const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                          const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                          char *out, uint64_t cap, uint64_t *used, bool sorted, uint32_t *order, bool bam = false,
                          int32_t nmCarryIn = 0, int32_t *nmCarryOut = nullptr) {
    if (int rc = enter(bam ? "bam_format" : "sam_format", a,
                       reads && ids && idOffsets && idLengths && results && editDistance && nOps && ops && used))
        return rc;
    if (int rc = snapgpu::samCheckClips(reads, nOps, &frontClipped, &unclippedLength)) return rc;
    if (bam)
        if (int rc = snapgpu::bamCheckIds(idLengths, reads->n)) return rc;
    HIPCHK(hipSetDevice(a->device));
    SamState &S = bam ? a->bamBatch : a->samBatch;
    hipStream_t st = a->sideStream;
    const uint64_t n = reads->n;
    if (S.ran && S.ev[1]) HIPCHK(hipEventSynchronize(S.ev[1]));
    uint64_t need = 0;
    for (uint64_t i = 0; i < n; i++)
        need = std::max<uint64_t>(need, unclippedLength ? reads->offsets[i] - frontClipped[i] + unclippedLength[i]
                                                        : reads->offsets[i] + reads->lengths[i]);
    samline::Args A;
    memset(&A, 0, sizeof(A));
    struct Up { DevBuf *b; const void *src; uint64_t bytes; };
    const Up ups[] = {{&S.bases, reads->bases, need}, {&S.quals, reads->quals, need},
                      {&S.res, results, n * sizeof(snapgpu_result_t)}, {&S.ed, editDistance, n * 4},
                      {&S.nOps, nOps, n * 4}, {&S.ops, ops, n * SNAPGPU_CIGAR_MAX_OPS * 4}};
    for (const Up &u : ups) {
        HIPCHK(devGrow(a, *u.b, u.bytes + 64));
        HIPCHK(hipMemsetAsync((char *)u.b->p + u.bytes, 0, 64, st));
        if (u.bytes) HIPCHK(hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, st));
    }
    A.bases = (const char *)S.bases.p;
    A.quals = (const char *)S.quals.p;
    A.res = (const snapgpu_result_t *)S.res.p;
    A.ed = (const int32_t *)S.ed.p;
    A.nOps = (const uint32_t *)S.nOps.p;
    A.ops = (const uint32_t *)S.ops.p;
    SamHostIn H;
    H.n = n; H.offsets = reads->offsets; H.lengths = reads->lengths;
    H.ids = ids; H.idOffsets = idOffsets; H.idLengths = idLengths;
    H.front = frontClipped; H.unclipped = unclippedLength; H.rg = readGroup;
    if (int rc = samPrepare(a, S, H, false, A)) return rc;
    if (int rc = bam ? bamLaunch(a, a->bamBatch, A, n, sorted, nmCarryIn) : samLaunch(a, S, A, n, sorted)) return rc;
    if (int rc = bam ? bamDownload(a, a->bamBatch, out, cap, used, nmCarryOut) : samDownload(a, S, out, cap, used)) return rc;
    return sorted && order ? samOrderDownload(a, S, order) : SNAPGPU_OK;
}

// ------------------------------------------------- BGZF on the device (bgzf.hip)
// The compressor's passes on the side stream over the bytes at `in`: their count is *nDev (the
// resident records' total, written by the BAM passes ahead on that stream) or n, at most capBytes.
static int bgzfLaunch(snapgpu_aligner_t *a, BgzfState &S, const char *in, const uint64_t *nDev, uint64_t n, uint64_t capBytes) {
    if (int rc = stageEvents(S)) return rc;
    S.ran = true;
    S.downloadMs = 0;
    a->last[kStageBgzf] = &S;
    S.maxBlocks = bgzfgpu::blocksOf(nDev ? capBytes : std::min(n, capBytes));
    S.empty = S.maxBlocks == 0;
    if (S.maxBlocks == 0) return SNAPGPU_OK;
    if (S.maxBlocks > 0x7fffffffull) { snapgpu::setError("bgzf: input too large"); return SNAPGPU_EINVAL; }
    if (!a->bgzfGrid) {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, a->device));
        a->bgzfGrid = std::max(1, prop.multiProcessorCount);
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(S.maxBlocks, (uint64_t)a->bgzfGrid);
    HIPCHK(devGrow(a, S.slots, S.maxBlocks * bgzfblock::kSlot));
    HIPCHK(devGrow(a, S.packed, S.maxBlocks * bgzfblock::kSlot));
    HIPCHK(devGrow(a, S.sizes, S.maxBlocks * 4));
    HIPCHK(devGrow(a, S.offs, (S.maxBlocks + 1) * 8));
    HIPCHK(devGrow(a, S.tokens, (uint64_t)grid * bgzfblock::kBlockIn * 4));
    HIPCHK(devGrow(a, S.res, sizeof(bgzfgpu::Result)));
    const bgzfgpu::Buffers B{(uint8_t *)S.slots.p, (uint32_t *)S.sizes.p, (uint64_t *)S.offs.p, (uint32_t *)S.tokens.p,
                             (uint8_t *)S.packed.p, (bgzfgpu::Result *)S.res.p, grid};
    HIPCHK(hipEventRecord(S.ev[0], a->sideStream));
    HIPCHK(bgzfgpu::launch((const uint8_t *)in, nDev, n, capBytes, B, a->sideStream, S.ev[1], S.ev[2]));
    HIPCHK(hipEventRecord(S.ev[3], a->sideStream));
    return SNAPGPU_OK;
}

// Wait for S's kernels, check them, and copy the packed members (and the EOF block) to the caller.
static int bgzfDownload(snapgpu_aligner_t *a, BgzfState &S, int eof, char *out, uint64_t cap, uint64_t *used) {
    static const unsigned char kEof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0,
                                           3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    *used = 0;
    S.downloadMs = 0;
    uint64_t total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (S.maxBlocks) {
        if (int rc = waitEvent(a, S.ev[3])) return rc;
        bgzfgpu::Result r{};
        HIPCHK(hipMemcpy(&r, S.res.p, sizeof r, hipMemcpyDeviceToHost));
        if (r.bad || r.nBlocks > S.maxBlocks || r.total > S.maxBlocks * bgzfblock::kSlot) {
            char msg[160];
            snprintf(msg, sizeof msg, "bgzf: %u of %u members are not what the size array says (stream %llu bytes, %llu slots)",
                     r.bad, r.nBlocks, (unsigned long long)r.total, (unsigned long long)S.maxBlocks);
            snapgpu::setError(msg);
            return SNAPGPU_EDEVICE;
        }
        total = r.total;
    }
    const uint64_t need = total + (eof ? 28 : 0);
    *used = need;
    if (need > cap || (!out && need)) { snapgpu::setError("bgzf_download: output buffer too small"); return SNAPGPU_EINVAL; }
    if (total)
        if (int rc = textDownload(a, (const char *)S.packed.p, total, out)) return rc;
    if (eof) memcpy(out + total, kEof, 28);
    S.downloadMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SNAPGPU_OK;
}

// ------------------------------------------------- the batch forms' records from the host
// The record starts (and n behind them): a walk over the block sizes on the host.
static int recordStarts(const char *who, const char *records, uint64_t n, std::vector<uint64_t> &starts) {
    for (uint64_t u = 0; u < n;) {
        starts.push_back(u);
        const uint64_t bytes = n - u < 4 ? 0 : (uint64_t)baiindex::load32((const uint8_t *)records + u) + 4;
        if (bytes < baiindex::kFixed || bytes > n - u) {
            snapgpu::setError(std::string(who) + ": record " + std::to_string(starts.size() - 1) + ": truncated");
            return SNAPGPU_EFORMAT;
        }
        u += bytes;
    }
    starts.push_back(n);
    return SNAPGPU_OK;
}

// The n bytes of records into `in` and their starts into `dStarts` on the side stream; waited for,
// so the host copies may go.
static int batchUpload(snapgpu_aligner_t *a, DevBuf &in, const char *records, uint64_t n, DevBuf &dStarts,
                       const std::vector<uint64_t> &starts) {
    HIPCHK(devGrow(a, in, n + 64));
    if (n) HIPCHK(hipMemcpyAsync(in.p, records, n, hipMemcpyHostToDevice, a->sideStream));
    HIPCHK(devGrow(a, dStarts, starts.size() * 8));
    HIPCHK(hipMemcpyAsync(dStarts.p, starts.data(), starts.size() * 8, hipMemcpyHostToDevice, a->sideStream));
    HIPCHK(hipStreamSynchronize(a->sideStream));
    return SNAPGPU_OK;
}

// ------------------------------------------------- BAI on the device (bai.hip)
// The index passes on the side stream over n records at text + start[i], members at coff.
static int baiLaunch(snapgpu_aligner_t *a, BaiState &S, const char *text, const uint64_t *start, uint64_t n, uint64_t recordBytes,
                     uint32_t nRef, const uint64_t *coff, uint64_t streamOffset) {
    if (int rc = stageEvents(S)) return rc;
    if (n > 0xfffffffeull) { snapgpu::setError("bai: batch too large"); return SNAPGPU_EINVAL; }
    // an earlier call's kernels may still use the buffers that grow
    if (S.launched) HIPCHK(hipEventSynchronize(S.ev[baigpu::kPasses]));
    S.ran = false;
    uint64_t temp = 0;
    HIPCHK(baigpu::tempBytes(n, a->sideStream, &temp));
    S.L = baigpu::layout(n, nRef, temp);
    S.outCap = (baiindex::sizeBound(n, nRef, recordBytes) + 15) & ~15ull;
    HIPCHK(devGrow(a, S.work, S.L.bytes));
    HIPCHK(devGrow(a, S.out, S.outCap));
    S.n = n;
    S.nRef = nRef;
    S.downloadMs = 0;
    a->last[kStageBai] = &S;
    HIPCHK(baigpu::launch((const uint8_t *)text, start, n, nRef, coff, streamOffset, (char *)S.work.p, S.L, (uint8_t *)S.out.p,
                          S.outCap, a->sideStream, S.ev));
    S.ran = S.launched = true;
    return SNAPGPU_OK;
}

// Wait for S's kernels, check them, and copy the index to the caller.
static int baiDownload(snapgpu_aligner_t *a, BaiState &S, char *out, uint64_t cap, uint64_t *used) {
    *used = 0;
    S.downloadMs = 0;
    if (int rc = waitEvent(a, S.ev[baigpu::kPasses])) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    baigpu::Result r{};
    HIPCHK(hipMemcpy(&r, (const char *)S.work.p + S.L.res, sizeof r, hipMemcpyDeviceToHost));
    if (r.bad || r.total > S.outCap) {
        char msg[200];
        snprintf(msg, sizeof msg, "bai: %u records are refused or out of (refID, pos) order, or the counts do not add up "
                                  "(index %llu bytes, bound %llu)", r.bad, (unsigned long long)r.total, (unsigned long long)S.outCap);
        snapgpu::setError(msg);
        return SNAPGPU_EDEVICE;
    }
    *used = r.total;
    if (r.total > cap || !out) { snapgpu::setError("bai_download: output buffer too small"); return SNAPGPU_EINVAL; }
    HIPCHK(hipMemcpy(out, S.out.p, r.total, hipMemcpyDeviceToHost));
    S.downloadMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SNAPGPU_OK;
}

// ------------------------------------------------- duplicate marking on the device (dupmark.hip)
// The mark passes on the side stream over n records at text + start[i].
static int dupLaunch(snapgpu_aligner_t *a, DupState &S, char *text, const uint64_t *start, uint64_t n, uint32_t nRef) {
    if (int rc = stageEvents(S)) return rc;
    if (n > 0xfffffffeull) { snapgpu::setError("dupmark: batch too large"); return SNAPGPU_EINVAL; }
    // an earlier call's kernels may still use the buffers that grow
    if (S.launched) HIPCHK(hipEventSynchronize(S.ev[dupgpu::kPasses]));
    S.ran = false;
    uint64_t temp = 0;
    HIPCHK(dupgpu::tempBytes(n, a->sideStream, &temp));
    S.L = dupgpu::layout(n, temp);
    HIPCHK(devGrow(a, S.work, S.L.bytes));
    S.downloadMs = 0;
    a->last[kStageDup] = &S;
    HIPCHK(dupgpu::launch((uint8_t *)text, start, n, nRef, (char *)S.work.p, S.L, a->sideStream, S.ev));
    S.ran = S.launched = true;
    return SNAPGPU_OK;
}

extern "C" {

int snapgpu_sam_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                         const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                         const char *readGroup) {
    return samResident(a, d, reads, ids, idOffsets, idLengths, readGroup, false);
}

int snapgpu_sam_resident_sorted(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                                const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                                const char *readGroup) {
    return samResident(a, d, reads, ids, idOffsets, idLengths, readGroup, true);
}

int snapgpu_sam_order_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint32_t *order) {
    return orderDownload("sam_order_download",
                         "sam_order_download: the batch's last SAM call was not snapgpu_sam_resident_sorted (or there was none)", a,
                         d ? &d->sam : nullptr, order);
}

int snapgpu_sam_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *out, uint64_t cap, uint64_t *used) {
    if (int rc = enter("sam_download", a, d && used)) return rc;
    if (!d->sam.ran) { snapgpu::setError("sam_download: no snapgpu_sam_resident before snapgpu_sam_download"); return SNAPGPU_EINVAL; }
    HIPCHK(hipSetDevice(a->device));
    return samDownload(a, d->sam, out, cap, used);
}

int snapgpu_sam_format_gpu(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                           const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                           const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                           const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                           char *out, uint64_t cap, uint64_t *used) {
    return samFormatBatch(a, reads, ids, idOffsets, idLengths, results, editDistance, nOps, ops, readGroup, frontClipped,
                          unclippedLength, out, cap, used, false, nullptr);
}

int snapgpu_sam_format_gpu_sorted(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                                  const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                                  const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                  const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                                  char *out, uint64_t cap, uint64_t *used, uint32_t *order) {
    return samFormatBatch(a, reads, ids, idOffsets, idLengths, results, editDistance, nOps, ops, readGroup, frontClipped,
                          unclippedLength, out, cap, used, true, order);
}

int snapgpu_sam_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs) {
    return stageLastMs(a, kStageSam, false, "sam_last_ms: no device SAM call on this aligner", 0, 1, kernelMs, downloadMs);
}

int snapgpu_sam_pass_ms(snapgpu_aligner_t *a, double *lengthMs, double *scanMs, double *writeMs) {
    if (!a || !lengthMs || !scanMs || !writeMs) return SNAPGPU_EINVAL;
    StageState *last;
    if (int rc = lastStage(a, kStageSam, false, "sam_pass_ms: no device SAM call on this aligner", &last)) return rc;
    SamState &S = *static_cast<SamState *>(last);
    float f[3] = {0, 0, 0};
    if (S.n) {
        HIPCHK(hipEventSynchronize(S.ev[1]));
        HIPCHK(hipEventElapsedTime(&f[0], S.ev[0], S.ev[2]));
        HIPCHK(hipEventElapsedTime(&f[1], S.sorted ? S.ev[4] : S.ev[2], S.ev[3]));   // the sort step is not the scan's
        HIPCHK(hipEventElapsedTime(&f[2], S.ev[3], S.ev[1]));
    }
    *lengthMs = f[0];
    *scanMs = f[1];
    *writeMs = f[2];
    return SNAPGPU_OK;
}

int snapgpu_sam_sort_ms(snapgpu_aligner_t *a, double *sortMs) {
    if (!a || !sortMs) return SNAPGPU_EINVAL;
    StageState *last;
    if (int rc = lastStage(a, kStageSam, false, "sam_sort_ms: no device SAM call on this aligner", &last)) return rc;
    SamState &S = *static_cast<SamState *>(last);
    float f = 0;
    if (S.n && S.sorted) {
        HIPCHK(hipEventSynchronize(S.ev[1]));
        HIPCHK(hipEventElapsedTime(&f, S.ev[2], S.ev[4]));
    }
    *sortMs = f;
    return SNAPGPU_OK;
}

int snapgpu_bam_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                         const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                         const char *readGroup, int32_t nmCarryIn) {
    return samResident(a, d, reads, ids, idOffsets, idLengths, readGroup, false, true, nmCarryIn);
}

int snapgpu_bam_resident_sorted(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                                const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                                const char *readGroup, int32_t nmCarryIn) {
    return samResident(a, d, reads, ids, idOffsets, idLengths, readGroup, true, true, nmCarryIn);
}

int snapgpu_bam_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *out, uint64_t cap, uint64_t *used,
                         int32_t *nmCarryOut) {
    if (int rc = enter("bam_download", a, d && used)) return rc;
    if (!d->bam.ran) { snapgpu::setError("bam_download: no snapgpu_bam_resident before snapgpu_bam_download"); return SNAPGPU_EINVAL; }
    HIPCHK(hipSetDevice(a->device));
    if (d->dup.ran) {   // the records are the marked ones: the mark passes have to be through, and sound
        dupgpu::Result r{};
        if (int rc = dupResult(a, d->dup, &r)) { *used = 0; return rc; }
    }
    return bamDownload(a, d->bam, out, cap, used, nmCarryOut);
}

int snapgpu_bam_order_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint32_t *order) {
    return orderDownload("bam_order_download",
                         "bam_order_download: the batch's last BAM call was not snapgpu_bam_resident_sorted (or there was none)", a,
                         d ? &d->bam : nullptr, order);
}

int snapgpu_bam_format_gpu(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                           const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                           const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                           const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                           int32_t nmCarryIn, int32_t *nmCarryOut, char *out, uint64_t cap, uint64_t *used, int sorted,
                           uint32_t *order) {
    return samFormatBatch(a, reads, ids, idOffsets, idLengths, results, editDistance, nOps, ops, readGroup, frontClipped,
                          unclippedLength, out, cap, used, sorted != 0, order, true, nmCarryIn, nmCarryOut);
}

int snapgpu_bam_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs) {
    return stageLastMs(a, kStageBam, false, "bam_last_ms: no device BAM call on this aligner", 0, 1, kernelMs, downloadMs);
}

int snapgpu_bam_bgzf_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d) {
    if (int rc = enter("bam_bgzf_resident", a, d != nullptr, d)) return rc;
    if (!d->bam.ran) {
        snapgpu::setError("bam_bgzf_resident: no snapgpu_bam_resident before snapgpu_bam_bgzf_resident");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    // the records and their total are written by the BAM passes ahead on the side stream; the next
    // snapgpu_bam_resident rewrites them on that stream, after these passes
    const BamState &R = d->bam;
    d->bai.ran = false;   // the member offsets change: an index over the earlier ones is stale
    if (R.n == 0) return bgzfLaunch(a, d->bgzf, nullptr, nullptr, 0, 0);
    return bgzfLaunch(a, d->bgzf, (const char *)R.text.p, (const uint64_t *)R.start.p + R.n, 0, R.textBound);
}

int snapgpu_bam_bgzf_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, int eof, char *out, uint64_t cap,
                              uint64_t *used) {
    if (int rc = enter("bam_bgzf_download", a, d && used)) return rc;
    if (!d->bgzf.ran) {
        snapgpu::setError("bam_bgzf_download: no snapgpu_bam_bgzf_resident since the batch's last snapgpu_bam_resident");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    return bgzfDownload(a, d->bgzf, eof, out, cap, used);
}

int snapgpu_bgzf_compress_gpu(snapgpu_aligner_t *a, const char *in, uint64_t n, int eof, char *out, uint64_t cap,
                              uint64_t *used) {
    if (int rc = enter("bgzf_compress_gpu", a, (in || !n) && used)) return rc;
    HIPCHK(hipSetDevice(a->device));
    BgzfState &S = a->bgzfBatch;
    if (S.ran && S.maxBlocks) HIPCHK(hipEventSynchronize(S.ev[3]));
    if (n) {
        HIPCHK(devGrow(a, S.in, n + 64));
        HIPCHK(hipMemcpyAsync(S.in.p, in, n, hipMemcpyHostToDevice, a->sideStream));
    }
    if (int rc = bgzfLaunch(a, S, (const char *)S.in.p, nullptr, n, n)) return rc;
    return bgzfDownload(a, S, eof, out, cap, used);
}

int snapgpu_bgzf_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs) {
    return stageLastMs(a, kStageBgzf, false, "bgzf_last_ms: no device BGZF call on this aligner", 0, 3, kernelMs, downloadMs);
}

// ms[0 .. 3): the compress pass, the scan, the gather pass with the check, of the last device BGZF
// call (tools/bgzf_gpu_time.py)
int snapgpu_internal_bgzf_pass_ms(snapgpu_aligner_t *a, double *ms) { return stagePassMs(a, kStageBgzf, false, ms); }

int snapgpu_bam_bai_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint64_t streamOffset) {
    if (int rc = enter("bam_bai_resident", a, d != nullptr, d)) return rc;
    if (!d->bam.ran || !d->bam.sorted) {
        snapgpu::setError("bam_bai_resident: the batch's last BAM call was not snapgpu_bam_resident_sorted (or there was none)");
        return SNAPGPU_EINVAL;
    }
    if (!d->bgzf.ran) {
        snapgpu::setError("bam_bai_resident: no snapgpu_bam_bgzf_resident since the batch's last snapgpu_bam_resident_sorted");
        return SNAPGPU_EINVAL;
    }
    if (streamOffset >= baiindex::kStreamOffsetLimit) {
        snapgpu::setError("bam_bai_resident: streamOffset does not fit a virtual offset");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    const BamState &R = d->bam;
    const uint32_t nRef = (uint32_t)a->idx->genome->pieceOffsets.size();
    return baiLaunch(a, d->bai, (const char *)R.text.p, (const uint64_t *)R.start.p, R.n, R.n ? R.textBound : 0, nRef,
                     (const uint64_t *)d->bgzf.offs.p, streamOffset);
}

int snapgpu_bam_bai_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *out, uint64_t cap, uint64_t *used) {
    if (int rc = enter("bam_bai_download", a, d && used)) return rc;
    if (!d->bai.ran) {
        snapgpu::setError("bam_bai_download: no snapgpu_bam_bai_resident since the batch's last snapgpu_bam_resident or "
                          "snapgpu_bam_bgzf_resident");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    return baiDownload(a, d->bai, out, cap, used);
}

int snapgpu_bai_build_gpu(snapgpu_aligner_t *a, const char *records, uint64_t n, int32_t nRef, uint64_t streamOffset,
                          char *bgzfOut, uint64_t bgzfCap, uint64_t *bgzfUsed, char *baiOut, uint64_t baiCap,
                          uint64_t *baiUsed) {
    if (!a || (!records && n) || !bgzfUsed || !baiUsed || nRef < 0) { snapgpu::setError("bai_build_gpu: bad argument"); return SNAPGPU_EINVAL; }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    if (streamOffset >= baiindex::kStreamOffsetLimit) {
        snapgpu::setError("bai_build_gpu: streamOffset does not fit a virtual offset");
        return SNAPGPU_EINVAL;
    }
    std::vector<uint64_t> starts;
    if (int rc = recordStarts("bai_build_gpu", records, n, starts)) return rc;
    const uint64_t nRec = starts.size() - 1;
    HIPCHK(hipSetDevice(a->device));
    BgzfState &Z = a->bgzfBatch;
    BaiState &S = a->baiBatch;
    if (Z.ran && Z.maxBlocks) HIPCHK(hipEventSynchronize(Z.ev[3]));
    if (S.launched) HIPCHK(hipEventSynchronize(S.ev[baigpu::kPasses]));
    S.ran = false;
    if (int rc = batchUpload(a, Z.in, records, n, S.starts, starts)) return rc;
    if (int rc = bgzfLaunch(a, Z, (const char *)Z.in.p, nullptr, n, n)) return rc;
    if (int rc = baiLaunch(a, S, (const char *)Z.in.p, (const uint64_t *)S.starts.p, nRec, n, (uint32_t)nRef,
                           (const uint64_t *)Z.offs.p, streamOffset))
        return rc;
    if (int rc = bgzfDownload(a, Z, 0, bgzfOut, bgzfCap, bgzfUsed)) return rc;
    return baiDownload(a, S, baiOut, baiCap, baiUsed);
}

int snapgpu_bai_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs) {
    return stageLastMs(a, kStageBai, true, "bai_last_ms: no device BAI call on this aligner", 0, baigpu::kPasses, kernelMs,
                       downloadMs);
}

// ms[0 .. baigpu::kPasses): the passes of the last device BAI call (tools/bai_time.py)
int snapgpu_internal_bai_pass_ms(snapgpu_aligner_t *a, double *ms) { return stagePassMs(a, kStageBai, true, ms); }

int snapgpu_bam_dupmark_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d) {
    if (int rc = enter("bam_dupmark_resident", a, d != nullptr, d)) return rc;
    if (!d->bam.ran || !d->bam.sorted) {
        snapgpu::setError("bam_dupmark_resident: the batch's last BAM call was not snapgpu_bam_resident_sorted (or there was none)");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    BamState &R = d->bam;
    const uint32_t nRef = (uint32_t)a->idx->genome->pieceOffsets.size();
    d->bgzf.ran = d->bai.ran = false;   // the records change: a compressed stream of the earlier ones, and its index, are stale
    if (int rc = dupLaunch(a, d->dup, (char *)R.text.p, (const uint64_t *)R.start.p, R.n, nRef)) return rc;
    // the next pass set over these reads rewrites the records: it waits for the mark kernels too
    HIPCHK(hipEventRecord(a->residentSideDone, a->sideStream));
    a->residentSidePending = true;
    return SNAPGPU_OK;
}

int snapgpu_bam_dupmark_stats(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint64_t *nMarked, uint64_t *nGroups) {
    if (int rc = enter("bam_dupmark_stats", a, d && nMarked && nGroups)) return rc;
    if (!d->dup.ran) {
        snapgpu::setError("bam_dupmark_stats: no snapgpu_bam_dupmark_resident since the batch's last snapgpu_bam_resident");
        return SNAPGPU_EINVAL;
    }
    HIPCHK(hipSetDevice(a->device));
    dupgpu::Result r{};
    *nMarked = *nGroups = 0;
    if (int rc = dupResult(a, d->dup, &r)) return rc;
    *nMarked = r.marked;
    *nGroups = r.groups;
    return SNAPGPU_OK;
}

int snapgpu_bam_mark_duplicates_gpu(snapgpu_aligner_t *a, char *records, uint64_t n, int32_t nRef, uint64_t *nMarked,
                                    uint64_t *nGroups) {
    if (!a || (!records && n) || !nMarked || !nGroups || nRef < 0) { snapgpu::setError("bam_mark_duplicates_gpu: bad argument"); return SNAPGPU_EINVAL; }
    if (a->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    *nMarked = *nGroups = 0;
    std::vector<uint64_t> starts;
    if (int rc = recordStarts("bam_mark_duplicates_gpu", records, n, starts)) return rc;
    const uint64_t nRec = starts.size() - 1;
    HIPCHK(hipSetDevice(a->device));
    DupState &S = a->dupBatch;
    if (S.launched) HIPCHK(hipEventSynchronize(S.ev[dupgpu::kPasses]));
    S.ran = false;
    if (int rc = batchUpload(a, S.in, records, n, S.starts, starts)) return rc;
    if (int rc = dupLaunch(a, S, (char *)S.in.p, (const uint64_t *)S.starts.p, nRec, (uint32_t)nRef)) return rc;
    dupgpu::Result r{};
    if (int rc = dupResult(a, S, &r)) return rc;   // the caller's records stay as they were
    const auto t0 = std::chrono::steady_clock::now();
    if (n) HIPCHK(hipMemcpy(records, S.in.p, n, hipMemcpyDeviceToHost));
    S.downloadMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *nMarked = r.marked;
    *nGroups = r.groups;
    return SNAPGPU_OK;
}

int snapgpu_bam_dupmark_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs) {
    return stageLastMs(a, kStageDup, true, "bam_dupmark_last_ms: no device duplicate marking on this aligner", 0,
                       dupgpu::kPasses, kernelMs, downloadMs);
}

// ms[0 .. dupgpu::kPasses): the passes of the last device duplicate marking (tools/dupmark_time.py)
int snapgpu_internal_dupmark_pass_ms(snapgpu_aligner_t *a, double *ms) { return stagePassMs(a, kStageDup, true, ms); }

}  // extern "C"
