// simple_align.h -- simple_align_kernel: the reads whose seeds all point at one candidate location,
// aligned without the general kernel's machinery.
//
// Most short reads map uniquely with few errors: every seed that hits at all hits the same (location,
// direction), the reference scores that one candidate once, and the rest of its seed loop only counts
// seeds until lowestPossibleScore passes the score limit.  align_kernel<128> runs its element hash,
// insertion batch, pop and in-order apply around that.  This kernel walks the read's pass-0 seed
// records (seed_lookup.h) with the control flow of align_one's seed loop, runs the one LV pass with
// the general scorer's own device code (the mask build of lv_pass, lv_group, lv_prob_groups: the same
// bits) and writes the full record.  Whatever it cannot be sure of it leaves alone: the read goes
// onto a list, nothing is written to `out`, and align_kernel<128> aligns the read from scratch.  A
// bail can therefore never change a result.
//
// What the general path would have carried and this kernel drops (one element, one candidate):
//  - the element's weight, sort key and chain link order pops and find elements: with one element
//    there is nothing to order or find, and it is popped by the score call of the seed that made it;
//  - its lps is tested against the score limit when it is popped: it was <= the limit when the
//    element was made (allowAlloc), and the limit does not change before that score call;
//  - candidatesUsed / candidatesScored / allScored: a later hit on the scored candidate leaves the
//    element all-scored, so it is never relinked and never scored again;
//  - the candidate's seed offset is overwritten by later hits, after the only LV pass that reads it;
//  - the nearby element of the success step does not exist;
//  - a hit on another location is dropped by the general path without a trace when it cannot
//    allocate (lps above the limit) and is not in the candidate's element: so here; any other second
//    location bails.
#pragma once
#include "align_score.h"
#include "seed_lookup.h"

namespace sgk {

struct SimpleLds {
    char fwd[128];                                  // read[FORWARD], zero slack
    char fwdQ[128];
    alignas(16) uint8_t rows8[MAX_K - 1][WAVE];     // LV rows 1..MAX_K-1 (lv_group)
    GroupLdsT<2> grp;                               // read planes and path slots (the scorer's layout)
};

enum : int { SIMPLE_DONE = 0, SIMPLE_BAIL = 1, SIMPLE_LONG = 2 };

// One read <= 128 bases.  SIMPLE_DONE: its record is written.  SIMPLE_BAIL: nothing is written.
// SIMPLE_LONG: a longer read, which pass 0 has put on pass 2's list.
__device__ __forceinline__ int simple_one(const KArgs &A, SimpleLds &S, uint32_t r) {
    auto &G = S.grp;
    const int lane = lane_id();
    const uint32_t n = A.lengths[r];
    if (n > 128u) return SIMPLE_LONG;
    const uint32_t seedLen = A.seedLen;
    if (n > A.maxReadSize || n < seedLen) return SIMPLE_BAIL;
    const uint64_t off = A.offsets[r];
    // Read::init upper-casing (align_one); any byte that is not ACGT bails
    bool other = false;
    wave_sync();
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int i = h * 64 + lane;
        uint32_t c = 0, q = 0;
        if (i < (int)n) {
            c = (uint8_t)A.bases[off + i];
            q = (uint8_t)A.quals[off + i];
            if (c >= 'a' && c <= 'z') c -= 0x20;
        }
        S.fwd[i] = (char)c;
        S.fwdQ[i] = (char)q;
        other |= ballot(i < (int)n && packed_code(c) > 3u) != 0;
    }
    wave_sync();
    if (other) return SIMPLE_BAIL;
    const uint32_t srec = ((const uint32_t *)(A.seedRecs + (uint64_t)r * SEEDS_PER_READ))[lane];
    const uint32_t maxSeeds = A.maxSeedsCmd ? A.maxSeedsCmd : A.tab->maxSeedsForLen[n];
    const uint32_t nPossible = n - seedLen + 1;
    // both directions apply every seed here (no popular seed without an overflow list), so lps and
    // nSeedsApplied are the same in both
    uint32_t lps = 0, nApplied = 0, seedsRcp = rcp16_of(1);
    uint32_t bestScore = UNUSED_SCORE, bestLoc = 0, scoreLimit = A.maxK + A.extra;
    double pAll = 0, pBest = 0;
    uint32_t outLoc = INVALID, outDir = 0;
    uint64_t used0 = 0, used1 = 0;   // BaseAligner::seedUsed, positions 0..63 and 64..127
    uint32_t next = 0, wrapCount = 0, pfIdx = 0;
    uint32_t nLookups = 0, nProbes = 0, nHitWords = 0, nScored = 0;
    bool haveElem = false;
    uint32_t candLoc = 0, candDir = 0;
    for (;;) {
        bool force = 2 * nApplied >= maxSeeds;
        if (!force && next >= nPossible) {
            wrapCount++;
            if (wrapCount >= seedLen) force = true;
            else {
                next = A.tab->wrap[wrapCount];
                seedsRcp = A.tab->rcp16[wrapCount + 1];
            }
        }
        bool linked = false;   // this seed made the element: the score call below pops it
        uint32_t s0 = 0;
        if (!force) {
            while (next < nPossible && (((next < 64 ? used0 : used1) >> (next & 63)) & 1)) next++;
            if (next >= nPossible) continue;
            if (next < 64) used0 |= 1ull << next; else used1 |= 1ull << (next & 63);
            if (pfIdx >= (uint32_t)SEEDS_PER_READ) return SIMPLE_BAIL;
            const uint32_t meta = readlaneu(srec, 4 * pfIdx);
            if (!((meta >> 31) && (meta & 0xff) == next && ((meta >> 16) & 0x7fff) != 0x7fff)) return SIMPLE_BAIL;
            const bool found = (meta >> 8) & 1, comp = (meta >> 9) & 1, pal = (meta >> 10) & 1;
            nProbes += (meta >> 16) & 0x7fff;
            const uint32_t v1 = readlaneu(srec, 4 * pfIdx + 1), v2 = readlaneu(srec, 4 * pfIdx + 2);
            pfIdx++;
            uint32_t nH[2] = {0, 0}, sg[2] = {0, 0};
            if (found) {
                if (pal) return SIMPLE_BAIL;
                const uint32_t vf = comp ? v2 : v1, vr = comp ? v1 : v2;
                if (vf < A.nBases) { nH[0] = 1; sg[0] = vf; }
                else if (vf != UNUSED_SIDE) return SIMPLE_BAIL;   // an overflow list
                if (vr < A.nBases) { nH[1] = 1; sg[1] = vr; }
                else if (vr != UNUSED_SIDE) return SIMPLE_BAIL;
            }
            nLookups++;
            nHitWords += nH[0] + nH[1];   // (maxHits >= 1: no hit is popular)
            // insert_hits, the forward hit then the reverse-complement one
#pragma unroll
            for (uint32_t dir = 0; dir < 2; dir++) {
                const uint32_t offset = dir ? n - seedLen - next : next;
                if (!nH[dir] || sg[dir] < offset) continue;
                const uint32_t loc = sg[dir] - offset;
                const bool allowAlloc = lps <= scoreLimit;
                if (!haveElem) {
                    if (!allowAlloc) continue;
                    haveElem = true; linked = true;
                    candLoc = loc; candDir = dir; s0 = offset;
                } else if (loc == candLoc && dir == candDir) {
                    // the scored candidate of the all-scored element: nothing changes
                } else if ((loc / ELEM == candLoc / ELEM && dir == candDir) || allowAlloc) {
                    return SIMPLE_BAIL;   // a second candidate
                }
            }
            nApplied++;
            next += seedLen;
        }
        // score(): lps_update, then the pop of what is linked
        {
            const uint32_t v = quot_rcp16(nApplied, seedsRcp);
            if (v > lps) lps = v;
        }
        const bool forced = force || lps > scoreLimit;
        if (linked) {
            if (!substring_ok(A, candLoc, n + MAX_K)) return SIMPLE_BAIL;
            // read bit planes {hi, lo, notACGT} of both directions (align_one)
#pragma unroll
            for (int dr = 0; dr < 2; dr++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int m = h * 64 + lane;
                    uint32_t code;
                    if (dr == 0) code = packed_code((uint8_t)S.fwd[m]);
                    else {
                        code = m < (int)n ? packed_code((uint8_t)S.fwd[n - 1 - m]) : 4u;
                        if (code < 4) code ^= 3u;
                    }
                    const uint64_t bh = ballot(code < 4 && (code & 2)), bl = ballot(code < 4 && (code & 1));
                    const uint64_t bm = ballot(code > 3);
                    if (lane == 0) { G.rpl[dr][0][h] = bh; G.rpl[dr][1][h] = bl; G.rpl[dr][2][h] = bm; }
                }
            wave_sync();
            const int k = (int)(scoreLimit < (uint32_t)(MAX_K - 1) ? scoreLimit : (uint32_t)(MAX_K - 1));
            constexpr int NW = 2, GS = 64, c = GS / 2 - 1;
            // F_x from the genome bit planes (lv_pass): positions loc + x + [0, 128), x = lane - c
            MaskW<NW> F;
            {
                const int64_t gp = (int64_t)candLoc + (lane - c) + PACK_GUARD;
                const GPlane *src = A.gpl + (gp >> 5);
                const uint32_t sh = (uint32_t)gp & 31;
                GPlane w[2 * NW + 1];
#pragma unroll
                for (int j = 0; j < 2 * NW + 1; j++) w[j] = src[j];
                const uint64_t *rp = &G.rpl[candDir][0][0];
                uint64_t RHw[NW], RLw[NW], RMw[NW];
#pragma unroll
                for (int j = 0; j < NW; j++) { RHw[j] = rp[j]; RLw[j] = rp[NW + j]; RMw[j] = rp[2 * NW + j]; }
                uint32_t f[2 * NW];
#pragma unroll
                for (int j = 0; j < 2 * NW; j++) {
                    const uint32_t gh = __builtin_amdgcn_alignbit(w[j + 1].hi, w[j].hi, sh);
                    const uint32_t gl = __builtin_amdgcn_alignbit(w[j + 1].lo, w[j].lo, sh);
                    const uint32_t gm = __builtin_amdgcn_alignbit(w[j + 1].nm, w[j].nm, sh);
                    const uint64_t RH = RHw[j / 2], RL = RLw[j / 2], RM = RMw[j / 2];
                    const uint32_t sft = 32 * (j & 1);
                    f[j] = (gh ^ (uint32_t)(RH >> sft)) | (gl ^ (uint32_t)(RL >> sft)) | gm | (uint32_t)(RM >> sft);
                }
#pragma unroll
                for (int j = 0; j < NW; j++) F.w[j] = ((uint64_t)f[2 * j + 1] << 32) | f[2 * j];
            }
            uint8_t (*rows)[WAVE] = reinterpret_cast<uint8_t (*)[WAVE]>(&S.rows8[0][0] - WAVE);
            const int s = (int)s0, t = s + (int)seedLen, glen = (int)n + MAX_K;
            int e1 = -1, e2 = -1;
            lv_group<1, GS, NW, true>(G, rows, F, true, t, (int)n - t, glen - t, k, k, e1);
            e1 = unii(e1);
            if (e1 < 0) return SIMPLE_BAIL;   // (a failed candidate stays in the general kernel)
            const int k2 = k - e1;
            {
                // reverse LV: pattern = read[s-1 .. 0], text = genome backwards from loc + s - 1
                const MaskW<NW> R = mk_reverse(F);
                lv_group<-1, GS, NW>(G, rows, R, true, 64 * NW - 1 - (s - 1), s, s + MAX_K, k2, k2, e2);
            }
            e2 = unii(e2);
            if (e2 < 0) return SIMPLE_BAIL;
            double qv = 1.0;
            int netv = 0;
            lv_prob_groups<GS, NW>(G, true, (int)n, s, (int)seedLen, candDir, S.fwdQ, qv, netv);
            // the success step of pass_apply on a fresh element with no nearby one
            const double q1 = readlaned(qv, 0), q2 = readlaned(qv, 32);
            const int net2 = readlane(netv, 32);
            const double prob = q1 * q2 * A.tab->seedProb;
            const uint32_t sc = (uint32_t)(e1 + e2);
            nScored = 1;
            pAll = 0.0 + prob;
            bestScore = sc;
            pBest = prob;
            bestLoc = candLoc + (uint32_t)net2;
            outLoc = bestLoc;
            outDir = candDir;
            scoreLimit = (bestScore < A.maxK ? bestScore : A.maxK) + A.extra;
        }
        if (forced) break;
    }
    // finalize_read
    uint32_t flags = 0;
    int result, mapq = 0;
    if (bestScore <= A.maxK) {
        outLoc = bestLoc;
        mapq = mapq_dev(A.tab, pAll, pBest, bestScore, 0u, &flags);
        result = mapq >= 10 ? SNAPGPU_SINGLE_HIT : SNAPGPU_MULTIPLE_HITS;
    } else {
        result = nApplied == 0 ? SNAPGPU_MULTIPLE_HITS : SNAPGPU_NOT_FOUND;
    }
    if (lane_id() == 0) {
        snapgpu_result_t o;
        o.location = outLoc;
        o.score = (int32_t)bestScore;
        o.mapq = mapq;
        o.result = (uint8_t)result;
        o.direction = (uint8_t)outDir;
        o.flags = (uint8_t)flags;
        o.reserved = 0;
        o.nLookups = nLookups;
        o.nLocationsScored = nScored;
        o.popularSeedsSkipped = 0;
        o.nHitsIgnored = 0;
        o.nProbes = nProbes;
        o.nHitWords = nHitWords;
        o.nOverflowLists = 0;
        o.nElements = haveElem ? 1u : 0u;
        o.reserved2 = 0;
        o.probabilityOfAllCandidates = pAll;
        o.probabilityOfBestCandidate = pBest;
        A.out[r] = o;
    }
    return SIMPLE_DONE;
}

// Persistent, one wave per read, over every read of the batch in input order.  A wave takes SIMPLE_CHUNK
// reads from the queue (A.counter) with one atomic and appends the chunk's bailed reads to `list` (for
// align_kernel<128>) with one more: a read costs this kernel so little that an atomic per read on one
// address would bound it.  *nDone counts the records written (one atomic per wave).
constexpr uint32_t SIMPLE_CHUNK = 8;
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void simple_align_kernel(KArgs A, uint32_t *list,
                                                                                                  uint32_t *listCount,
                                                                                                  uint32_t *nDone) {
    __shared__ SimpleLds S;
    uint32_t done = 0;
    for (;;) {
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(A.counter, SIMPLE_CHUNK);
        base = uni((uint32_t)readlane((int)base, 0));
        if (base >= A.nReads) break;
        if (__hip_atomic_load(&A.diag[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;   // watchdog: drain
        const uint32_t end = A.nReads - base < SIMPLE_CHUNK ? A.nReads : base + SIMPLE_CHUNK;
        uint32_t bailed = 0;   // bit j: read base + j bailed
        for (uint32_t i = base; i < end; i++) {
            if (i == A.tripRead && lane_id() == 0) diag_report(A.diag, DIAG_TEST_TRIP, i, 0);   // test hook
            const int rc = simple_one(A, S, i);
            if (rc == SIMPLE_BAIL) bailed |= 1u << (i - base);
            else if (rc == SIMPLE_DONE) done++;
        }
        if (bailed) {
            const int lane = lane_id();
            const uint32_t nb = (uint32_t)__builtin_popcount(bailed);
            uint32_t pos = 0;
            if (lane == 0) pos = atomicAdd(listCount, nb);
            pos = uni((uint32_t)readlane((int)pos, 0));
            uint32_t m = bailed;   // lane l writes the l-th bailed read of the chunk
            for (int j = 0; j < lane && j < (int)SIMPLE_CHUNK; j++) m &= m - 1;
            if ((uint32_t)lane < nb) list[pos + (uint32_t)lane] = base + (uint32_t)__builtin_ctz(m);
        }
    }
    if (done && lane_id() == 0) atomicAdd(nDone, done);
}

}  // namespace sgk
