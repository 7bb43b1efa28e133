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
#include "simple_schedule.h"

namespace sgk {

struct SimpleLds {
    char fwd[128];                                  // read[FORWARD], zero slack
    char fwdQ[128];
    alignas(16) uint8_t rows8[MAX_K - 1][WAVE];     // LV rows 1..MAX_K-1 (lv_group)
    GroupLdsT<2> grp;                               // read planes and path slots (the scorer's layout)
};
// grp.ecache and grp.cand belong to the general kernel's batches; here they hold the four-read path's
// per-group qualities and read planes and the wave's buffer of bailed reads (below)
__device__ __forceinline__ uint64_t *quad_quals(SimpleLds &S) {    // [4][16]: read g's qualities, bytes 0..127
    return reinterpret_cast<uint64_t *>(&S.grp.ecache[0][0]);
}
__device__ __forceinline__ uint32_t *bail_buf(SimpleLds &S) {      // [64]
    return reinterpret_cast<uint32_t *>(&S.grp.cand[0]);
}
__device__ __forceinline__ uint64_t *quad_planes(SimpleLds &S) {   // [4][3][2]: read g's forward {hi, lo, notACGT}
    return reinterpret_cast<uint64_t *>(&S.grp.cand[128]);
}
static_assert(sizeof(GroupLdsT<2>::ecache) >= 4 * 128 && sizeof(GroupLdsT<2>::cand) >= 256 + 4 * 48, "quad overlays");
static_assert(offsetof(GroupLdsT<2>, ecache) % 8 == 0 && offsetof(GroupLdsT<2>, cand) % 8 == 0, "quad overlays: 8-B words");

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

// ------------------------------------------------------------ four reads per wave
// simple_one is a chain of about fifteen dependent memory round trips with nothing to cover them.  The
// quad path runs four reads per wave, read g in lanes 16g .. 16g+15, lane 16g+k holding seed record k:
//  1. lengths, offsets and the four reads' records in one batch of loads;
//  2. bases, qualities and the walk schedule (DevTables::simpleSched, simple_schedule.h);
//  3. the walk as per-lane predicates and ballots inside the group: for an all-ACGT read the k-th
//     visited seed is seedSeq[n][k] and lowestPossibleScore around step k is the schedule's, so the
//     records decide only where the walk stops, which step links and whether the read bails;
//  4. the genome planes, and one narrow LV pass (lv_group<., 16, 2> at limit <= QUAD_K, the general
//     scorer's 16-lane form: the same score, path and probability bits as any group size);
//  5. the probability factors (lv_prob_groups<16, 2>) and the record.
// It writes a record only where it has reproduced simple_one, bails only where simple_one provably
// bails (a flagged record the walk reaches, a second candidate, an unservable window, a failed LV when
// the narrow limit is the whole limit) and hands everything else to simple_one: QUAD_ONE.
constexpr int QUAD_K = 7;   // rows of a 16-lane LV group (GS / 2 - 1)
enum : int { QUAD_NONE = 3, QUAD_ONE = 4 };

// the bits of this lane's 16-lane group in a wave ballot
__device__ __forceinline__ uint32_t group_bits(bool p, int gi) { return (uint32_t)(ballot(p) >> (16 * gi)) & 0xffffu; }
// the bits of x up to and including its lowest set one (x != 0)
__device__ __forceinline__ uint32_t upto_lowest(uint32_t x) { return x ^ (x - 1u); }
// sum over the lane's row of 16, in every lane of it (sum_reduce32's row steps)
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);   // row_mirror
    return v;
}
// the dwords of the aligned run holding bytes [a, a + nb), nb <= 8, as the 8 bytes from a (no dword without
// one of those bytes is read)
__device__ __forceinline__ uint64_t load8(const char *p, int nb) {
    // (the pointer minus its low bits: an address rounded through an integer loses its address space, a flat load)
    const uint32_t lead = (uint32_t)(uint64_t)p & 3u, sh = 8u * lead;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p - lead);
    uint32_t w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = 4 * i < (int)lead + nb ? src[i] : 0u;
    const uint32_t d0 = __builtin_amdgcn_alignbit(w[1], w[0], sh), d1 = __builtin_amdgcn_alignbit(w[2], w[1], sh);
    return ((uint64_t)d1 << 32) | d0;
}

// Reads r0 .. r0+3 (below `end`).  Returns this lane's group's code: SIMPLE_DONE (record written),
// SIMPLE_BAIL, SIMPLE_LONG, QUAD_ONE (for simple_one) or QUAD_NONE (no read).
__device__ __forceinline__ int simple_quad(const KArgs &A, SimpleLds &S, uint32_t r0, uint32_t end) {
    auto &G = S.grp;
    const int lane = lane_id();
    const int gi = lane >> 4, k = lane & 15;
    const uint32_t r = r0 + (uint32_t)gi;
    const bool have = r < end;
    const uint32_t seedLen = A.seedLen;
    // ---- round trip 1
    uint32_t n = 0;
    uint64_t off = 0;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (have) {
        n = A.lengths[r];
        off = A.offsets[r];
        rec = A.seedRecs[(uint64_t)r * SEEDS_PER_READ + (uint32_t)k];
    }
    if (have && k == 0 && r == A.tripRead) diag_report(A.diag, DIAG_TEST_TRIP, r, 0);   // test hook
    int code = !have ? QUAD_NONE : n > 128u ? SIMPLE_LONG : (n > A.maxReadSize || n < seedLen) ? QUAD_ONE : -1;
    // ---- round trip 2
    const DevTables *tab = A.tab;
    const uint32_t nt = code < 0 ? n : 0u;   // (row 0 of the tables: no seed, no step)
    const uint32_t seq = tab->seedSeq[nt][k];
    const uint32_t lpsA = tab->simpleSched[nt][k];
    const uint32_t stp = tab->simpleSteps[nt];
    const int nIn = (int)nt - 8 * k;   // this lane's eight read positions 8k .. 8k+7: those inside the read
    uint64_t b8 = 0, q8 = 0;
    if (nIn > 0) {
        b8 = load8(A.bases + off + 8u * (uint32_t)k, nIn < 8 ? nIn : 8);
        q8 = load8(A.quals + off + 8u * (uint32_t)k, nIn < 8 ? nIn : 8);
    }
    // Read::init upper-casing, the bit-plane code (packed_code) and ACGT membership per byte, as seed_lookup.h
    uint32_t hi8 = 0, lo8 = 0, nm8 = 0;
    bool bad = false;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const uint32_t c = (uint32_t)(b8 >> (8 * b)) & 0xffu;
        const uint32_t uc = (c >= 'a' && c <= 'z') ? c - 0x20u : c;
        const uint32_t o = uc - 0x40u;
        constexpr uint32_t kAcgt = (1u << 1) | (1u << 3) | (1u << 7) | (1u << 20);   // A C G T
        const bool inside = b < nIn;
        const bool acgt = inside && o < 32u && ((kAcgt >> (o & 31u)) & 1u);
        const uint32_t x0 = (uc >> 1) & 1u, x1 = (uc >> 2) & 1u;   // bits 2:1 of the letter: A 00, C 01, G 11, T 10
        bad |= inside && !acgt;
        hi8 |= (acgt ? x1 : 0u) << b;            // A 0, C 0, G 1, T 1
        lo8 |= (acgt ? x0 ^ x1 : 0u) << b;       // A 0, C 1, G 0, T 1
        nm8 |= (acgt ? 0u : 1u) << b;
    }
    if (nIn < 8) q8 &= nIn > 0 ? (1ull << (8 * nIn)) - 1ull : 0ull;
    wave_sync();
    {
        uint8_t *pl = reinterpret_cast<uint8_t *>(quad_planes(S) + 6 * gi);
        pl[k] = (uint8_t)hi8;
        pl[16 + k] = (uint8_t)lo8;
        pl[32 + k] = (uint8_t)nm8;
        quad_quals(S)[16 * gi + k] = q8;
    }
    wave_sync();
    const uint32_t badG = group_bits(bad, gi);
    if (code < 0 && badG) code = QUAD_ONE;   // a byte that is not ACGT: the sequence is not the table's
    // ---- the walk
    const uint32_t SL0 = A.maxK + A.extra, X = A.extra;
    const uint32_t nSteps = stp & 0x7fu;
    const bool need17 = (stp >> 7) != 0;
    const uint32_t stepsM = (1u << nSteps) - 1u;
    const uint32_t lpsB = (uint32_t)__builtin_amdgcn_mov_dpp((int)lpsA, 0x111, 0xf, 0xf, true);   // row_shr:1 (step 0: 0)
    const uint32_t meta = rec.x;
    const uint32_t probes = (meta >> 16) & 0x7fffu;
    const bool recOK = (meta >> 31) && seq != 0xffu && (meta & 0xffu) == seq && probes != 0x7fffu;
    const bool found = (meta >> 8) & 1, comp = (meta >> 9) & 1, pal = (meta >> 10) & 1;
    const uint32_t vf = comp ? rec.z : rec.y, vr = comp ? rec.y : rec.z;
    const bool hF = found && vf < A.nBases, hR = found && vr < A.nBases;
    // a palindrome or an overflow list on either side: simple_one bails when it visits the step
    const bool flag = found && (pal || (!hF && vf != UNUSED_SIDE) || (!hR && vr != UNUSED_SIDE));
    const uint32_t offF = seq, offR = n - seedLen - seq;
    const bool uF = hF && vf >= offF, uR = hR && vr >= offR;   // usable hits (insert_hits)
    const uint32_t locF = vf - offF, locR = vr - offR;
    // before the link the limit is SL0: the walk visits the steps up to the first whose lps passes it
    const uint32_t mGt0 = group_bits(lpsA > SL0, gi) & stepsM;
    const uint32_t V0 = mGt0 ? stepsM & upto_lowest(mGt0) : stepsM;
    const uint32_t U = group_bits(uF || uR, gi) & V0;
    const uint32_t Bm = group_bits(flag, gi), Im = group_bits(!recOK, gi);
    const bool linkG = U != 0;
    const uint32_t Vpre = linkG ? V0 & upto_lowest(U) : V0;   // visited up to the link step j
    const int jl = (lane & 48) + (linkG ? (int)__builtin_ctz(U) : 0);
    if (code < 0) {
        if (Bm & Vpre) code = SIMPLE_BAIL;
        else if (Im & Vpre) code = QUAD_ONE;
    }
    // the link step's candidate (the forward hit first), in every lane of the group
    const uint32_t candLoc = (uint32_t)shfl_idx((int)(uF ? locF : locR), jl);
    const uint32_t jp = (uint32_t)shfl_idx((int)((uF ? offF : offR) | (uF ? 0u : 1u) << 8 | (uF && uR ? 1u : 0u) << 9 |
                                                 (lpsB > SL0 ? 1u : 0u) << 10 | (lpsA > SL0 ? 1u : 0u) << 11), jl);
    const uint32_t s0 = jp & 0xffu, candDir = (jp >> 8) & 1u;
    const bool endAtJ = (jp >> 11) & 1u;   // forced at the link step, with the limit before its LV pass
    if (code < 0 && linkG) {
        if ((jp >> 10) & 1u) code = QUAD_ONE;          // (no element above the limit; the walk has ended before)
        else if ((jp >> 9) & 1u) code = SIMPLE_BAIL;   // the step's reverse-complement hit: a second candidate
        else if (!substring_ok(A, candLoc, n + MAX_K)) code = SIMPLE_BAIL;
    }
    // later hits: the candidate again (nothing), its element and direction (bail), another location
    // (bail while lps before the step is within the limit, else dropped)
    bool c2any, c2lim;
    {
        const bool sameF = uF && locF == candLoc && candDir == 0u, sameR = uR && locR == candLoc && candDir == 1u;
        const bool elF = uF && locF / ELEM == candLoc / ELEM && candDir == 0u;
        const bool elR = uR && locR / ELEM == candLoc / ELEM && candDir == 1u;
        c2any = (elF && !sameF) || (elR && !sameR);
        c2lim = (uF && !elF) || (uR && !elR);
    }
    const uint32_t after = linkG ? stepsM & ~upto_lowest(U) : 0u;   // the steps behind the link step
    const uint32_t C2a = group_bits(c2any, gi);
    {
        // whatever the LV pass returns the limit stays >= extraSearchDepth: what that shortest walk meets
        const uint32_t mGtX = group_bits(lpsA > X, gi) & after;
        const uint32_t Vmin = endAtJ ? 0u : (mGtX ? after & upto_lowest(mGtX) : after);
        const uint32_t C2x = group_bits(c2lim && lpsB <= X, gi);
        if (code < 0 && linkG) {
            if ((Bm | C2a | C2x) & Vmin) code = SIMPLE_BAIL;
            else if (Im & Vmin) code = QUAD_ONE;
        }
    }
    // ---- the LV pass of the groups that linked
    const bool live = code < 0 && linkG;
    bool okLV = false;
    uint32_t sc = 0, bestLoc = 0;
    double prob = 0.0;
    if (ballot(live) != 0) {
        constexpr int NW = 2, c = QUAD_K;
        const int nn = live ? (int)n : 128;
        MaskW<NW> F;
        {
            // F_x from the genome bit planes (lv_pass): positions loc + x + [0, 128), x = k - c
            const int64_t gp = (int64_t)(live ? candLoc : 0u) + (k - c) + PACK_GUARD;
            const GPlane *src = A.gpl + (gp >> 5);
            const uint32_t sh = (uint32_t)gp & 31;
            GPlane w[2 * NW + 1];
#pragma unroll
            for (int j = 0; j < 2 * NW + 1; j++) w[j] = src[j];
            // the read's planes in the candidate's direction: the forward ones, or -- every base is ACGT --
            // their complement, reversed over the read's n positions (simple_one's build of read[RC])
            const uint64_t *rp = quad_planes(S) + 6 * gi;
            uint64_t RHw[NW], RLw[NW], RMw[NW];
#pragma unroll
            for (int j = 0; j < NW; j++) { RHw[j] = rp[j]; RLw[j] = rp[NW + j]; RMw[j] = rp[2 * NW + j]; }
            if (candDir) {
                const uint32_t s = 128u - (uint32_t)nn;   // 0 .. 112
#pragma unroll
                for (int pln = 0; pln < 2; pln++) {
                    uint64_t *P = pln ? RLw : RHw;
                    const uint64_t b0 = brev64(~P[1] & ~RMw[1]), b1 = brev64(~P[0] & ~RMw[0]);   // reversed 128 bits
                    P[0] = s == 0 ? b0 : s < 64 ? (b0 >> (s & 63)) | (b1 << ((64 - s) & 63)) : b1 >> ((s - 64) & 63);
                    P[1] = s < 64 ? b1 >> (s & 63) : 0ull;
                }
            }
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
        // at a limit <= QUAD_K this is simple_one's pass; above it, its results wherever it succeeds (an LV call
        // with limit k' returns what a limit k >= k' returns when the answer is <= k')
        const int kq = (int)(SL0 < (uint32_t)QUAD_K ? SL0 : (uint32_t)QUAD_K);
        const int s = (int)s0, t = s + (int)seedLen;
        int e1 = -1, e2 = -1;
        lv_group<1, 16, NW, true>(G, rows, F, live, t, nn - t, nn + MAX_K - t, kq, kq, e1);
        const bool ract = live && e1 >= 0;
        const int k2 = kq - e1;
        const int kmax2 = (int)max_reduce32(ract ? (uint32_t)(k2 + 1) : 0u) - 1;   // largest reverse limit
        if (kmax2 >= 0) {
            // reverse LV: pattern = read[s-1 .. 0], text = genome backwards from loc + s - 1
            const MaskW<NW> R = mk_reverse(F);
            lv_group<-1, 16, NW>(G, rows, R, ract, 64 * NW - 1 - (s - 1), s, s + MAX_K, k2, kmax2, e2);
        }
        okLV = ract && e2 >= 0;
        // (a failed candidate stays in the general kernel; above the narrow limit simple_one decides)
        if (live && !okLV) code = SL0 <= (uint32_t)QUAD_K ? SIMPLE_BAIL : QUAD_ONE;
        if (ballot(okLV) != 0) {
            // lv_prob_groups' lanes: direction lane >> 5, path slots of group (lane & 31) / 8
            const int pg = (lane & 31) >> 3;
            const int pk = shfl_idx((okLV ? 1 : 0) | (int)candDir << 1 | s << 2 | nn << 10, 16 * pg);
            double qv = 1.0;
            int netv = 0;
            lv_prob_groups<16, NW>(G, (pk & 1) != 0, pk >> 10, (pk >> 2) & 0xff, (int)seedLen, (uint32_t)(pk >> 1) & 1u,
                                   reinterpret_cast<const char *>(quad_quals(S) + 16 * pg), qv, netv);
            // the success step of pass_apply on a fresh element with no nearby one, per group
            const uint64_t qb = (uint64_t)__double_as_longlong(qv);
            const int l1 = 8 * gi, l2 = 32 + 8 * gi;
            const double q1 = __longlong_as_double((long long)(((uint64_t)(uint32_t)shfl_idx((int)(uint32_t)(qb >> 32), l1) << 32) |
                                                               (uint32_t)shfl_idx((int)(uint32_t)qb, l1)));
            const double q2 = __longlong_as_double((long long)(((uint64_t)(uint32_t)shfl_idx((int)(uint32_t)(qb >> 32), l2) << 32) |
                                                               (uint32_t)shfl_idx((int)(uint32_t)qb, l2)));
            const int net2 = shfl_idx(netv, l2);
            prob = q1 * q2 * tab->seedProb;
            sc = (uint32_t)(e1 + e2);
            bestLoc = candLoc + (uint32_t)net2;
        }
    }
    // ---- the rest of the walk, with the limit the LV pass left
    const uint32_t SL1 = (sc < A.maxK ? sc : A.maxK) + X;
    const uint32_t mGt1 = group_bits(lpsA > SL1, gi) & after;
    const uint32_t Vpost = endAtJ ? 0u : (mGt1 ? after & upto_lowest(mGt1) : after);
    const uint32_t C21 = group_bits(c2lim && lpsB <= SL1, gi);
    const bool scored = code < 0 && linkG;   // (okLV)
    if (scored) {
        if ((Bm | C2a | C21) & Vpost) code = SIMPLE_BAIL;
        else if (Im & Vpost) code = QUAD_ONE;
    }
    // a walk that neither the limit nor the loop-top force ended asks for record 16
    const bool limitEnd = scored ? endAtJ || mGt1 != 0 : mGt0 != 0;
    if (code < 0 && need17 && !limitEnd) code = QUAD_ONE;
    const uint32_t V = scored ? Vpre | Vpost : V0;   // the steps visited: nLookups, nProbes, nHitWords over them
    const uint32_t sums = row_sum((V >> k) & 1u ? probes | ((hF ? 1u : 0u) + (hR ? 1u : 0u)) << 24 : 0u);
    if (code < 0) {
        const uint32_t nLook = (uint32_t)__builtin_popcount(V);
        // finalize_read
        const uint32_t bestScore = scored ? sc : UNUSED_SCORE;
        const double pAll = scored ? 0.0 + prob : 0.0, pBest = scored ? prob : 0.0;
        uint32_t flags = 0;
        int result, mapq = 0;
        if (bestScore <= A.maxK) {
            mapq = mapq_dev(tab, pAll, pBest, bestScore, 0u, &flags);
            result = mapq >= 10 ? SNAPGPU_SINGLE_HIT : SNAPGPU_MULTIPLE_HITS;
        } else {
            result = nLook == 0 ? SNAPGPU_MULTIPLE_HITS : SNAPGPU_NOT_FOUND;
        }
        if (k == 0) {
            snapgpu_result_t o;
            o.location = scored ? bestLoc : INVALID;
            o.score = (int32_t)bestScore;
            o.mapq = mapq;
            o.result = (uint8_t)result;
            o.direction = (uint8_t)(scored ? candDir : 0u);
            o.flags = (uint8_t)flags;
            o.reserved = 0;
            o.nLookups = nLook;
            o.nLocationsScored = scored ? 1u : 0u;
            o.popularSeedsSkipped = 0;
            o.nHitsIgnored = 0;
            o.nProbes = sums & 0xffffffu;
            o.nHitWords = sums >> 24;
            o.nOverflowLists = 0;
            o.nElements = scored ? 1u : 0u;
            o.reserved2 = 0;
            o.probabilityOfAllCandidates = pAll;
            o.probabilityOfBestCandidate = pBest;
            A.out[r] = o;
        }
        code = SIMPLE_DONE;
    }
    return code;
}

// Persistent, over every read of the batch in input order.  A wave takes SIMPLE_CHUNK reads from the queue
// (A.counter) with one atomic and runs them four at a time (simple_quad), then one at a time those the quad
// path handed on (simple_one; *nWide counts the records that path writes).  The bailed reads collect in an
// LDS buffer and go onto `list` (for align_kernel<128>) with one atomic per 32 or more of them and a last
// flush: the queue and the list are one address each, and an atomic per eight reads on either would bound a
// kernel this short.  *nDone counts the records written (one atomic per wave).
constexpr uint32_t SIMPLE_CHUNK = 32;
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void simple_align_kernel(KArgs A, uint32_t *list,
                                                                                                  uint32_t *listCount,
                                                                                                  uint32_t *nDone,
                                                                                                  uint32_t *nWide) {
    __shared__ SimpleLds S;
    uint32_t done = 0, wide = 0, nBuf = 0;
    for (;;) {
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(A.counter, SIMPLE_CHUNK);
        base = uni((uint32_t)readlane((int)base, 0));
        bool stop = base >= A.nReads;
        if (!stop && __hip_atomic_load(&A.diag[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) stop = true;   // watchdog: drain
        if (!stop) {
            const uint32_t end = A.nReads - base < SIMPLE_CHUNK ? A.nReads : base + SIMPLE_CHUNK;
            for (uint32_t q0 = base; q0 < end; q0 += 4) {
                const int code = simple_quad(A, S, q0, end);
                const int lane = lane_id();
                const bool lead = (lane & 15) == 0;
                done += (uint32_t)__popcll(ballot(lead && code == SIMPLE_DONE));
                const uint64_t bm = ballot(lead && code == SIMPLE_BAIL);
                if (lead && code == SIMPLE_BAIL)
                    bail_buf(S)[nBuf + (uint32_t)__popcll(bm & ((1ull << lane) - 1))] = q0 + (uint32_t)(lane >> 4);
                nBuf += (uint32_t)__popcll(bm);
                uint64_t om = ballot(lead && code == QUAD_ONE);
                while (om) {   // the quad's LDS is free: its records are written
                    const uint32_t i = q0 + ((uint32_t)__builtin_ctzll(om) >> 4);
                    om &= om - 1;
                    const int rc = simple_one(A, S, i);
                    if (rc == SIMPLE_BAIL) {
                        if (lane_id() == 0) bail_buf(S)[nBuf] = i;
                        nBuf++;
                    } else if (rc == SIMPLE_DONE) { done++; wide++; }
                }
            }
        }
        // at most 31 entries stay behind a chunk, so the next chunk's 32 fit the buffer's 64
        if (nBuf >= 32u || (stop && nBuf)) {
            const int lane = lane_id();
            wave_sync();
            uint32_t pos = 0;
            if (lane == 0) pos = atomicAdd(listCount, nBuf);
            pos = uni((uint32_t)readlane((int)pos, 0));
            if ((uint32_t)lane < nBuf) list[pos + (uint32_t)lane] = bail_buf(S)[lane];
            wave_sync();
            nBuf = 0;
        }
        if (stop) break;
    }
    if (lane_id() == 0) {
        if (done) atomicAdd(nDone, done);
        if (wide) atomicAdd(nWide, wide);
    }
}

}  // namespace sgk
