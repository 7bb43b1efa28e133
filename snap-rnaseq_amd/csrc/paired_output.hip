// paired_output.hip -- the host side of the paired aligner's output calls behind include/snapgpu.h:
// CIGARs of both ends of the resident pair batch (cigar_kernel over the bases the intersecting run
// left in HBM, where they are), the pairs' SAM text (sam_pair_format.hip) and their BAM records
// (bam_pair_format.hip, in write order or coordinate order), over the resident batch and in a batch
// form.  No kernels here.  The state is the single-end text stage's (SamState) with what only pairs
// have, the records' a BamState beside it, and their buffer growth, packed upload, check and
// download are the single-end chain's (aligner_state.h, output_chain.hip).  Everything is queued on
// the paired aligner's one stream, so the next intersecting run's copies into the read buffers wait
// for these kernels by stream order; that run marks the CIGARs, the text and the records stale
// (pairedOutputStale).  Buffers are grow-only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "aligner_state.h"
#include "bam_pair_format.h"
#include "paired_state.h"
#include "sam_pair_format.h"

// SamState's members as the pair uses them: res, ed, nOps, ops are the CIGAR pass's copy of the
// caller's pair records and its 2n rows, each end's n entries a plane (entry e * n + q); aux and the
// text passes' buffers as they are (aux: both ends' ids and clip arrays, and the batch form's read
// offsets and lengths); n = the 2n records of the last SAM launch; ev[0..1] around the SAM passes,
// `launched`: they were recorded.  It is nobody's a->last[]: snapgpu_paired_sam_last_ms reports it.
struct PairedOutput : SamState {
    static constexpr int kCigarEv = 5;   // ev[5..6] around the CIGAR pass
    DevBuf cgLoc, cgDir;                 // cigar_kernel's 2n locations and directions, planes as the rows
    // the batch form's reads, records and CIGAR rows (the resident batch's stay as they are)
    DevBuf bBases[2], bQuals[2], bRes, bEd, bNOps, bOps;
    std::vector<uint32_t> hLen[2];    // the resident batch's lengths, fetched by the CIGAR pass
    bool cigarsValid = false;         // the rows are those of the resident batch
    bool textValid = false;           // the text is that of the resident batch and its rows
    bool cigarTimed = false;          // ev[5..6] were recorded
    // The BAM records' own aux upload, pass buffers and output (n = the 2n records of the last BAM
    // launch, ev[0..1] around its passes, sorted / order, carryIn): the text above stays what it is.
    BamState bam;
    bool bamValid = false;            // the records are those of the resident batch and its rows
    PairedOutput() : SamState(kStageSam, kCigarEv + 2) {
        bufs.insert(bufs.end(), {&cgLoc, &cgDir, &bBases[0], &bBases[1], &bQuals[0], &bQuals[1], &bRes, &bEd, &bNOps, &bOps});
    }
};

void pairedOutputStale(snapgpu_paired_aligner_t *pa) {
    pa->residentN = 0;
    if (pa->output) pa->output->cigarsValid = pa->output->textValid = pa->output->bamValid = false;
}

void pairedOutputFree(snapgpu_paired_aligner_t *pa) {
    PairedOutput *O = pa->output;
    if (!O) return;
    stageFree(pa->single, O->bam);
    stageFree(pa->single, *O);
    delete O;
    pa->output = nullptr;
}

namespace {

constexpr uint64_t kRowBytes = SNAPGPU_CIGAR_MAX_OPS * 4ull;   // one CIGAR row

// What every entry point begins with: 0, or the code to return (the message is set); *O = the state.
int enter(const char *who, snapgpu_paired_aligner_t *pa, bool argsOk, PairedOutput **O) {
    if (!pa || !argsOk) { snapgpu::setError(std::string(who) + ": null argument"); return SNAPGPU_EINVAL; }
    if (pa->single->failed) { snapgpu::setError("aligner failed earlier (device timeout)"); return SNAPGPU_EDEVICE; }
    HIPCHK(hipSetDevice(pa->device));
    if (!pa->output) pa->output = new PairedOutput();
    *O = pa->output;
    if (int rc = stageEvents((*O)->bam)) return rc;
    return stageEvents(**O);
}

// The formatters' check of one end's batch (ids, the 1024-base limit, its own clip state) -> the
// clip arrays, or both null.
int checkEnd(const char *who, const snapgpu_reads_t *r, const uint32_t **front, const uint32_t **unclipped) {
    if (r->n && (!r->ids || !r->idOffsets || !r->idLengths)) {
        snapgpu::setError(std::string(who) + ": a read batch carries no ids");
        return SNAPGPU_EINVAL;
    }
    *front = *unclipped = nullptr;
    return snapgpu::samCheckClips(r, nullptr, front, unclipped);
}

// Upload what the line rule needs beside reads, records and CIGAR rows into O.aux and point A at
// it: per end the ids, id offsets and lengths and the clip arrays (withExtents: the read offsets and
// lengths too), the piece names, the read group.  O.textBound = a bound on the bytes of text, which
// exceeds the BAM records' bytes (per record the id, 1.5 bytes per base and at most 36 + 1 + 4 * 66 +
// 4 + 15 more, plus the read group).  O: the text state, or the records' (PairedOutput::bam).
int samPrepare(snapgpu_paired_aligner_t *pa, SamState &O, const snapgpu_reads_t *const R[2],
               const uint32_t *const front[2], const uint32_t *const unclipped[2], const char *rg, bool withExtents,
               samline::PairArgs &A) {
    snapgpu_aligner_t *a = pa->single;
    const uint64_t n = R[0]->n;
    const snapgpu::Genome &g = *a->idx->genome;
    std::vector<uint32_t> nameOff;
    std::string names;
    snapgpu::samPieceNames(g, nameOff, names);
    const uint32_t rgLen = rg ? (uint32_t)strlen(rg) : 0u;
    uint32_t maxName = 1;
    for (size_t p = 0; p + 1 < nameOff.size(); p++) maxName = std::max(maxName, nameOff[p + 1] - nameOff[p]);
    // per line: flags, POS, MAPQ, PNEXT, TLEN, tabs, tags and NM (< 96), RNAME and RNEXT, two soft
    // clips and SNAPGPU_CIGAR_MAX_OPS ops of at most 11 bytes each
    const uint64_t perLine = 96 + 2ull * maxName + (rg ? 6 + rgLen : 0) + 22 + 11ull * SNAPGPU_CIGAR_MAX_OPS;
    uint64_t bound = 0, idBytes[2] = {0, 0};
    for (int e = 0; e < 2; e++)
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t len = unclipped[e] ? unclipped[e][i] : R[e]->lengths[i];
            bound += R[e]->idLengths[i] + 2ull * std::min(len, samline::kMaxSeq) + perLine;
            idBytes[e] = std::max<uint64_t>(idBytes[e], R[e]->idOffsets[i] + R[e]->idLengths[i]);
        }
    O.textBound = bound;
    // an earlier call's upload may still read hAux, its kernels aux
    if (O.launched) HIPCHK(hipEventSynchronize(O.ev[1]));
    AuxPack P;
    uint64_t oIdOff[2], oIdLen[2], oFront[2] = {0, 0}, oFull[2] = {0, 0}, oOff[2] = {0, 0}, oLen[2] = {0, 0}, oIds[2];
    for (int e = 0; e < 2; e++) {
        oIdOff[e] = P.add(R[e]->idOffsets, n * 8);
        oIdLen[e] = P.add(R[e]->idLengths, n * 4);
        if (unclipped[e]) { oFront[e] = P.add(front[e], n * 4); oFull[e] = P.add(unclipped[e], n * 4); }
        if (withExtents) { oOff[e] = P.add(R[e]->offsets, n * 8); oLen[e] = P.add(R[e]->lengths, n * 4); }
        oIds[e] = P.add(R[e]->ids, idBytes[e]);
    }
    const uint64_t oNameOff = P.add(nameOff.data(), nameOff.size() * 4), oNames = P.add(names.data(), names.size()),
                   oRg = P.add(rg, rgLen);
    P.copyTo(O.hAux);
    HIPCHK(devGrow(a, O.aux, O.hAux.size()));
    HIPCHK(hipMemcpyAsync(O.aux.p, O.hAux.data(), O.hAux.size(), hipMemcpyHostToDevice, pa->stream));
    const char *d = (const char *)O.aux.p;
    for (int e = 0; e < 2; e++) {
        A.idOffsets[e] = (const uint64_t *)(d + oIdOff[e]);
        A.idLengths[e] = (const uint32_t *)(d + oIdLen[e]);
        A.front[e] = unclipped[e] ? (const uint32_t *)(d + oFront[e]) : nullptr;
        A.unclipped[e] = unclipped[e] ? (const uint32_t *)(d + oFull[e]) : nullptr;
        if (withExtents) { A.offsets[e] = (const uint64_t *)(d + oOff[e]); A.lengths[e] = (const uint32_t *)(d + oLen[e]); }
        A.ids[e] = d + oIds[e];
    }
    A.pieceOffsets = a->dPieces;
    A.pieceNameOff = (const uint32_t *)(d + oNameOff);
    A.pieceNames = d + oNames;
    A.nPieces = (int32_t)g.pieceOffsets.size();
    A.rg = rg ? d + oRg : nullptr;
    A.rgLen = rgLen;
    return SNAPGPU_OK;
}

// Length pass, scan, write pass and check of the 2n records of n > 0 pairs on the aligner's stream.
int samLaunch(snapgpu_paired_aligner_t *pa, PairedOutput &O, const samline::PairArgs &A, uint64_t n) {
    samgpu::Buffers B;
    if (int rc = textBuffers(pa->single, O, 2 * n, &B)) return rc;
    O.n = 2 * n;
    HIPCHK(hipEventRecord(O.ev[0], pa->stream));
    HIPCHK(sampairgpu::launch(A, 2 * n, B, pa->stream));
    HIPCHK(hipEventRecord(O.ev[1], pa->stream));
    O.launched = true;
    return SNAPGPU_OK;
}

// Wait for the SAM passes, check them, and copy the text to the caller's buffer: the text is
// complete, so the single-end aligner's pinned staging (and its idle side stream) carry it.
int samDownload(snapgpu_paired_aligner_t *pa, PairedOutput &O, char *out, uint64_t cap, uint64_t *used) {
    return textFinish(pa->single, O, {"paired sam: %u of %llu lines do not end where the scan placed them (text %llu bytes, bound %llu)",
                                      "paired_sam_download"}, out, cap, used);
}

// The batch forms' check of their arguments (the host formatters'): *front / *unclipped per end.
int batchCheck(const char *who, snapgpu_paired_aligner_t *pa, const snapgpu_index_t *idx, const snapgpu_reads_t *const R[2],
               const snapgpu_pair_result_t *results, const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
               const uint32_t *front[2], const uint32_t *unclipped[2]) {
    if (idx && idx != pa->single->idx) {
        snapgpu::setError(std::string(who) + ": the index is not the paired aligner's");
        return SNAPGPU_EINVAL;
    }
    if (R[0]->n != R[1]->n) {
        snapgpu::setError(std::string(who) + ": the two read batches differ in length");
        return SNAPGPU_EINVAL;
    }
    const uint64_t n = R[0]->n;
    if (n && (!results || !editDistance || !nOps || !ops)) {
        snapgpu::setError(std::string(who) + ": null argument");
        return SNAPGPU_EINVAL;
    }
    for (int e = 0; e < 2; e++)
        if (int rc = checkEnd(who, R[e], &front[e], &unclipped[e])) return rc;
    for (uint64_t i = 0; i < 2 * n; i++)
        if (nOps[i] > SNAPGPU_CIGAR_MAX_OPS) {
            snapgpu::setError("sam_format: nOps > SNAPGPU_CIGAR_MAX_OPS, read longer than 1024 bases or bad clip arrays");
            return SNAPGPU_EINVAL;
        }
    return SNAPGPU_OK;
}

// The batch forms' reads, records and CIGAR rows of n > 0 pairs into their own buffers (queued on
// the aligner's stream), and A pointed at them: row 2q + e.
int batchUpload(snapgpu_paired_aligner_t *pa, PairedOutput &O, const snapgpu_reads_t *const R[2],
                const snapgpu_pair_result_t *results, const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                samline::PairArgs &A) {
    snapgpu_aligner_t *a = pa->single;
    hipStream_t st = pa->stream;
    const uint64_t n = R[0]->n, recs = 2 * n;
    memset(&A, 0, sizeof(A));
    for (int e = 0; e < 2; e++) {
        const uint64_t bytes = R[e]->totalBytes;
        HIPCHK(devGrow(a, O.bBases[e], bytes + 64));
        HIPCHK(devGrow(a, O.bQuals[e], bytes + 64));
        HIPCHK(hipMemcpyAsync(O.bBases[e].p, R[e]->bases, bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(O.bQuals[e].p, R[e]->quals, bytes, hipMemcpyHostToDevice, st));
        A.bases[e] = (const char *)O.bBases[e].p;
        A.quals[e] = (const char *)O.bQuals[e].p;
    }
    HIPCHK(devGrow(a, O.bRes, n * sizeof(snapgpu_pair_result_t)));
    HIPCHK(devGrow(a, O.bEd, recs * 4));
    HIPCHK(devGrow(a, O.bNOps, recs * 4));
    HIPCHK(devGrow(a, O.bOps, recs * kRowBytes));
    HIPCHK(hipMemcpyAsync(O.bRes.p, results, n * sizeof(snapgpu_pair_result_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(O.bEd.p, editDistance, recs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(O.bNOps.p, nOps, recs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(O.bOps.p, ops, recs * kRowBytes, hipMemcpyHostToDevice, st));
    A.res = (const snapgpu_pair_result_t *)O.bRes.p;
    A.ed = (const int32_t *)O.bEd.p; A.nOps = (const uint32_t *)O.bNOps.p; A.ops = (const uint32_t *)O.bOps.p;
    A.rowPair = 2; A.rowEnd = 1;
    return SNAPGPU_OK;
}

// The resident calls' check of their batches against the resident one (n, totalBytes, lengths) and
// of each end (checkEnd), and A pointed at the resident reads, the uploaded records and the CIGAR rows.
int residentArgs(const char *who, snapgpu_paired_aligner_t *pa, PairedOutput &O, const snapgpu_reads_t *const R[2],
                 const uint32_t *front[2], const uint32_t *unclipped[2], samline::PairArgs &A) {
    const uint64_t n = pa->residentN;
    if (!n) {
        snapgpu::setError(std::string(who) + ": no pair batch is resident (align a batch first)");
        return SNAPGPU_EINVAL;
    }
    if (!O.cigarsValid) {
        snapgpu::setError(std::string(who) + ": no snapgpu_paired_cigar_resident before it");
        return SNAPGPU_EINVAL;
    }
    for (int e = 0; e < 2; e++) {
        if (R[e]->n != n || R[e]->totalBytes != pa->residentBytes[e] ||
            memcmp(R[e]->lengths, O.hLen[e].data(), n * 4) != 0) {
            snapgpu::setError(std::string(who) + ": the reads batches do not match the resident batch (n, totalBytes or lengths differ)");
            return SNAPGPU_EINVAL;
        }
        if (int rc = checkEnd(who, R[e], &front[e], &unclipped[e])) return rc;
    }
    memset(&A, 0, sizeof(A));
    for (int e = 0; e < 2; e++) { A.bases[e] = pa->dB[e]; A.quals[e] = pa->dQ[e]; A.offsets[e] = pa->dO[e]; A.lengths[e] = pa->dL[e]; }
    A.res = (const snapgpu_pair_result_t *)O.res.p;
    A.ed = (const int32_t *)O.ed.p; A.nOps = (const uint32_t *)O.nOps.p; A.ops = (const uint32_t *)O.ops.p;
    A.rowPair = 1; A.rowEnd = n;   // as the CIGAR pass left them
    return SNAPGPU_OK;
}

// The encoder's passes over the 2n records of n > 0 pairs on the aligner's stream, into S's buffers
// (S.textBound: samPrepare's); sorted: in the stable order of the records' coordinate-sort keys
// (S.order keeps that order).
int bamLaunch(snapgpu_paired_aligner_t *pa, BamState &S, const samline::PairArgs &A, uint64_t n, bool sorted, int32_t nmCarryIn) {
    snapgpu_aligner_t *a = pa->single;
    const uint64_t recs = 2 * n;
    if (recs > 0xffffffffull) { snapgpu::setError("batch too large"); return SNAPGPU_EINVAL; }
    S.n = recs;
    S.sorted = sorted;
    S.carryIn = nmCarryIn;
    HIPCHK(devGrow(a, S.len, recs * 4));
    HIPCHK(devGrow(a, S.nm, recs * 4));
    HIPCHK(devGrow(a, S.nmTiles, samgpu::scanTiles(recs) * 4));
    HIPCHK(devGrow(a, S.start, (recs + 1) * 8));
    HIPCHK(devGrow(a, S.sums, samgpu::scanTiles(recs) * 8));
    HIPCHK(devGrow(a, S.bad, 16));
    HIPCHK(devGrow(a, S.text, S.textBound + 16));
    const bamgpu::Buffers B{(uint32_t *)S.len.p, (int32_t *)S.nm.p, (int32_t *)S.nmTiles.p, (uint64_t *)S.start.p,
                            (uint64_t *)S.sums.p, (char *)S.text.p, S.textBound, (uint32_t *)S.bad.p};
    samgpu::SortBuffers SB{};
    if (sorted)
        if (int rc = sortBuffers(a, S, recs, &SB)) return rc;
    HIPCHK(hipEventRecord(S.ev[0], pa->stream));
    HIPCHK(bampairgpu::launch(A, recs, nmCarryIn, B, pa->stream, sorted ? &SB : nullptr));
    HIPCHK(hipEventRecord(S.ev[1], pa->stream));
    S.launched = true;
    return SNAPGPU_OK;
}

// textFinish over the records, and the carry-out (the NM of the last record in write order): the
// carry-in again unless the check passed.
int bamDownload(snapgpu_paired_aligner_t *pa, BamState &S, char *out, uint64_t cap, uint64_t *used, int32_t *nmCarryOut) {
    if (nmCarryOut) *nmCarryOut = S.carryIn;
    auto carryOut = [](SamState &B, void *to) -> int {
        if (to) HIPCHK(hipMemcpy(to, (const int32_t *)static_cast<BamState &>(B).nm.p + B.n - 1, 4, hipMemcpyDeviceToHost));
        return SNAPGPU_OK;
    };
    return textFinish(pa->single, S, {"paired bam: %u of %llu records do not carry the size the scan gave them (output %llu bytes, bound %llu)",
                                      "paired_bam_download"}, out, cap, used, carryOut, nmCarryOut);
}

int bamResident(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1, const char *readGroup,
                int32_t nmCarryIn, bool sorted) {
    PairedOutput *Op;
    if (int rc = enter("paired_bam_resident", pa, reads0 && reads1, &Op)) return rc;
    PairedOutput &O = *Op;
    const snapgpu_reads_t *R[2] = {reads0, reads1};
    const uint32_t *front[2], *unclipped[2];
    samline::PairArgs A;
    if (int rc = residentArgs("paired_bam_resident", pa, O, R, front, unclipped, A)) return rc;
    if (int rc = snapgpu::bamCheckPairIds(reads0, reads1)) return rc;
    O.bamValid = false;
    if (int rc = samPrepare(pa, O.bam, R, front, unclipped, readGroup, false, A)) return rc;
    if (int rc = bamLaunch(pa, O.bam, A, pa->residentN, sorted, nmCarryIn)) return rc;
    O.bamValid = true;
    return SNAPGPU_OK;
}

}  // namespace

extern "C" {

uint64_t snapgpu_paired_resident_pairs(const snapgpu_paired_aligner_t *pa) { return pa ? pa->residentN : 0; }

int snapgpu_paired_cigar_resident(snapgpu_paired_aligner_t *pa, const snapgpu_pair_result_t *results, int useM) {
    PairedOutput *Op;
    if (int rc = enter("paired_cigar_resident", pa, results != nullptr, &Op)) return rc;
    PairedOutput &O = *Op;
    snapgpu_aligner_t *a = pa->single;
    const uint64_t n = pa->residentN;
    if (!n) {
        snapgpu::setError("paired_cigar_resident: no pair batch is resident (align a batch first)");
        return SNAPGPU_EINVAL;
    }
    O.cigarsValid = O.textValid = O.bamValid = false;
    hipStream_t st = pa->stream;
    const uint64_t recs = 2 * n;
    HIPCHK(devGrow(a, O.res, n * sizeof(snapgpu_pair_result_t)));
    HIPCHK(devGrow(a, O.cgLoc, recs * 4));
    HIPCHK(devGrow(a, O.cgDir, recs));
    HIPCHK(devGrow(a, O.ed, (recs + 1) * 4));
    HIPCHK(devGrow(a, O.nOps, (recs + 1) * 4));
    HIPCHK(devGrow(a, O.ops, (recs + 1) * kRowBytes));
    // the records up, the resident lengths down (snapgpu_paired_sam_resident compares its batch with
    // them), and waited for: the caller's array may go
    for (int e = 0; e < 2; e++) {
        O.hLen[e].resize(n);
        HIPCHK(hipMemcpyAsync(O.hLen[e].data(), pa->dL[e], n * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(O.res.p, results, n * sizeof(snapgpu_pair_result_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventRecord(O.ev[O.kCigarEv], st));
    // one cigar_kernel launch per end, over that end's resident reads where they are; end e's
    // locations, directions and rows are entries e * n + q (the line rule reads them there)
    sampairgpu::cigarInputs((const snapgpu_pair_result_t *)O.res.p, n, (uint32_t *)O.cgLoc.p, (uint8_t *)O.cgDir.p, st);
    HIPCHK(hipGetLastError());
    for (uint64_t e = 0; e < 2; e++)
        if (int rc = snapgpu_internal_cigar_device(a, st, pa->dB[e], pa->dO[e], pa->dL[e], n, (const uint32_t *)O.cgLoc.p + e * n,
                                                   (const uint8_t *)O.cgDir.p + e * n, useM, (int32_t *)O.ed.p + e * n,
                                                   (uint32_t *)O.nOps.p + e * n,
                                                   (uint32_t *)O.ops.p + e * n * SNAPGPU_CIGAR_MAX_OPS))
            return rc;
    HIPCHK(hipEventRecord(O.ev[O.kCigarEv + 1], st));
    O.cigarsValid = O.cigarTimed = true;
    return SNAPGPU_OK;
}

int snapgpu_paired_cigar_download(snapgpu_paired_aligner_t *pa, int32_t *editDistance, uint32_t *nOps, uint32_t *ops) {
    PairedOutput *O;
    if (int rc = enter("paired_cigar_download", pa, editDistance && nOps && ops, &O)) return rc;
    if (!O->cigarsValid) {
        snapgpu::setError("paired_cigar_download: no snapgpu_paired_cigar_resident on the resident batch");
        return SNAPGPU_EINVAL;
    }
    if (int rc = waitEvent(pa->single, O->ev[O->kCigarEv + 1])) return rc;
    // the device keeps each end's rows as a plane; the caller gets row 2q + e
    const uint64_t n = pa->residentN, recs = 2 * n;
    std::vector<uint32_t> h(recs * SNAPGPU_CIGAR_MAX_OPS);
    HIPCHK(hipMemcpy(h.data(), O->ed.p, recs * 4, hipMemcpyDeviceToHost));
    for (uint64_t e = 0; e < 2; e++)
        for (uint64_t q = 0; q < n; q++) editDistance[2 * q + e] = (int32_t)h[e * n + q];
    HIPCHK(hipMemcpy(h.data(), O->nOps.p, recs * 4, hipMemcpyDeviceToHost));
    for (uint64_t e = 0; e < 2; e++)
        for (uint64_t q = 0; q < n; q++) nOps[2 * q + e] = h[e * n + q];
    HIPCHK(hipMemcpy(h.data(), O->ops.p, recs * kRowBytes, hipMemcpyDeviceToHost));
    for (uint64_t e = 0; e < 2; e++)
        for (uint64_t q = 0; q < n; q++)
            memcpy(ops + (2 * q + e) * SNAPGPU_CIGAR_MAX_OPS, h.data() + (e * n + q) * SNAPGPU_CIGAR_MAX_OPS, kRowBytes);
    return SNAPGPU_OK;
}

int snapgpu_paired_sam_resident(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1,
                                const char *readGroup) {
    PairedOutput *Op;
    if (int rc = enter("paired_sam_resident", pa, reads0 && reads1, &Op)) return rc;
    PairedOutput &O = *Op;
    const snapgpu_reads_t *R[2] = {reads0, reads1};
    const uint32_t *front[2], *unclipped[2];
    samline::PairArgs A;
    if (int rc = residentArgs("paired_sam_resident", pa, O, R, front, unclipped, A)) return rc;
    O.textValid = false;
    if (int rc = samPrepare(pa, O, R, front, unclipped, readGroup, false, A)) return rc;
    if (int rc = samLaunch(pa, O, A, pa->residentN)) return rc;
    O.textValid = true;
    return SNAPGPU_OK;
}

int snapgpu_paired_sam_download(snapgpu_paired_aligner_t *pa, char *out, uint64_t cap, uint64_t *used) {
    PairedOutput *O;
    if (int rc = enter("paired_sam_download", pa, used != nullptr, &O)) return rc;
    *used = 0;
    if (!O->textValid) {
        snapgpu::setError("paired_sam_download: no snapgpu_paired_sam_resident on the resident batch");
        return SNAPGPU_EINVAL;
    }
    return samDownload(pa, *O, out, cap, used);
}

int snapgpu_paired_sam_last_ms(snapgpu_paired_aligner_t *pa, double *cigarMs, double *kernelMs, double *downloadMs) {
    PairedOutput *O;
    if (int rc = enter("paired_sam_last_ms", pa, cigarMs && kernelMs && downloadMs, &O)) return rc;
    float c = 0, k = 0;
    if (O->cigarTimed) {
        HIPCHK(hipEventSynchronize(O->ev[O->kCigarEv + 1]));
        HIPCHK(hipEventElapsedTime(&c, O->ev[O->kCigarEv], O->ev[O->kCigarEv + 1]));
    }
    if (O->launched) {
        HIPCHK(hipEventSynchronize(O->ev[1]));
        HIPCHK(hipEventElapsedTime(&k, O->ev[0], O->ev[1]));
    }
    *cigarMs = c;
    *kernelMs = k;
    *downloadMs = O->downloadMs;
    return SNAPGPU_OK;
}

int snapgpu_sam_format_pairs_gpu(snapgpu_paired_aligner_t *pa, const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                 const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results,
                                 const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                 const char *readGroup, char *out, uint64_t cap, uint64_t *used) {
    PairedOutput *Op;
    if (int rc = enter("sam_format_pairs_gpu", pa, reads0 && reads1 && used, &Op)) return rc;
    PairedOutput &O = *Op;
    *used = 0;
    const snapgpu_reads_t *R[2] = {reads0, reads1};
    const uint32_t *front[2], *unclipped[2];
    if (int rc = batchCheck("sam_format_pairs_gpu", pa, idx, R, results, editDistance, nOps, ops, front, unclipped)) return rc;
    const uint64_t n = reads0->n;
    if (n == 0) return SNAPGPU_OK;
    O.textValid = false;   // the text buffers take this call's lines
    samline::PairArgs A;
    if (int rc = batchUpload(pa, O, R, results, editDistance, nOps, ops, A)) return rc;
    if (int rc = samPrepare(pa, O, R, front, unclipped, readGroup, true, A)) return rc;
    if (int rc = samLaunch(pa, O, A, n)) return rc;
    return samDownload(pa, O, out, cap, used);
}

int snapgpu_paired_bam_resident(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1,
                                const char *readGroup, int32_t nmCarryIn) {
    return bamResident(pa, reads0, reads1, readGroup, nmCarryIn, false);
}

int snapgpu_paired_bam_resident_sorted(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0,
                                       const snapgpu_reads_t *reads1, const char *readGroup, int32_t nmCarryIn) {
    return bamResident(pa, reads0, reads1, readGroup, nmCarryIn, true);
}

int snapgpu_paired_bam_download(snapgpu_paired_aligner_t *pa, char *out, uint64_t cap, uint64_t *used, int32_t *nmCarryOut) {
    PairedOutput *O;
    if (int rc = enter("paired_bam_download", pa, used != nullptr, &O)) return rc;
    *used = 0;
    if (!O->bamValid) {
        snapgpu::setError("paired_bam_download: no snapgpu_paired_bam_resident on the resident batch");
        return SNAPGPU_EINVAL;
    }
    return bamDownload(pa, O->bam, out, cap, used, nmCarryOut);
}

int snapgpu_paired_bam_order_download(snapgpu_paired_aligner_t *pa, uint32_t *order) {
    PairedOutput *O;
    if (int rc = enter("paired_bam_order_download", pa, order != nullptr, &O)) return rc;
    if (!O->bamValid || !O->bam.sorted) {
        snapgpu::setError("paired_bam_order_download: the last resident BAM call was not a sorted one");
        return SNAPGPU_EINVAL;
    }
    if (int rc = waitEvent(pa->single, O->bam.ev[1])) return rc;
    HIPCHK(hipMemcpy(order, O->bam.order.p, O->bam.n * 4, hipMemcpyDeviceToHost));
    return SNAPGPU_OK;
}

int snapgpu_paired_bam_last_ms(snapgpu_paired_aligner_t *pa, double *kernelMs, double *downloadMs) {
    PairedOutput *O;
    if (int rc = enter("paired_bam_last_ms", pa, kernelMs && downloadMs, &O)) return rc;
    float k = 0;
    if (O->bam.launched) {
        HIPCHK(hipEventSynchronize(O->bam.ev[1]));
        HIPCHK(hipEventElapsedTime(&k, O->bam.ev[0], O->bam.ev[1]));
    }
    *kernelMs = k;
    *downloadMs = O->bam.downloadMs;
    return SNAPGPU_OK;
}

int snapgpu_bam_format_pairs_gpu(snapgpu_paired_aligner_t *pa, const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                 const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results,
                                 const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                 const char *readGroup, int32_t nmCarryIn, int32_t *nmCarryOut, char *out, uint64_t cap,
                                 uint64_t *used, int sorted, uint32_t *order) {
    PairedOutput *Op;
    if (int rc = enter("bam_format_pairs_gpu", pa, reads0 && reads1 && used, &Op)) return rc;
    PairedOutput &O = *Op;
    *used = 0;
    if (nmCarryOut) *nmCarryOut = nmCarryIn;
    const snapgpu_reads_t *R[2] = {reads0, reads1};
    const uint32_t *front[2], *unclipped[2];
    if (int rc = batchCheck("bam_format_pairs_gpu", pa, idx, R, results, editDistance, nOps, ops, front, unclipped)) return rc;
    if (int rc = snapgpu::bamCheckPairIds(reads0, reads1)) return rc;
    const uint64_t n = reads0->n;
    if (n == 0) return SNAPGPU_OK;
    O.bamValid = false;   // the record buffers take this call's records
    samline::PairArgs A;
    if (int rc = batchUpload(pa, O, R, results, editDistance, nOps, ops, A)) return rc;
    if (int rc = samPrepare(pa, O.bam, R, front, unclipped, readGroup, true, A)) return rc;
    if (int rc = bamLaunch(pa, O.bam, A, n, sorted != 0, nmCarryIn)) return rc;
    if (int rc = bamDownload(pa, O.bam, out, cap, used, nmCarryOut)) return rc;
    if (sorted && order) HIPCHK(hipMemcpy(order, O.bam.order.p, 2 * n * 4, hipMemcpyDeviceToHost));
    return SNAPGPU_OK;
}

}  // extern "C"
