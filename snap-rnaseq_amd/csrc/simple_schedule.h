// simple_schedule.h -- the seed walk of simple_one (simple_align.h) for a read whose bases are all ACGT,
// as a function of the read length alone.
//
// For such a read the k-th seed the walk visits is DevTables::seedSeq[n][k] and nSeedsApplied before
// step k is k, so lowestPossibleScore before and after every step, and the step at which the loop-top
// test (2 * nSeedsApplied >= maxSeeds, or the wrap count reaching seedLen) ends a walk that nothing else
// ended, depend on (n, seedLen, maxSeeds) only.  Lookup results decide where the walk stops before that,
// which step makes the element and whether the read bails: with this table those are per-lane predicates
// over a read's 16 seed records (simple_quad, simple_align.h).
//
// simple_schedule() replays the integer arithmetic of simple_one's loop -- which is align_one's -- with
// "no seed hits and no limit is exceeded".  Plain C++ (host and device; tests/c/simple_schedule_test.cpp
// compares it with a transcription of the loop for every n, four seed lengths and four maxSeeds).
#pragma once
#include <stdint.h>
#include "small_div.h"

namespace sgk {

constexpr int SCHED_STEPS = 16;   // = SEEDS_PER_READ (seed_lookup.h): the records a read has

struct SimpleSchedule {
    uint8_t lpsAfter[SCHED_STEPS];   // lowestPossibleScore after the score call of step k (lpsBefore[k] is
                                     // lpsAfter[k - 1], 0 for k = 0); steps >= nSteps repeat the last value
    uint8_t nSteps;                  // seeds visited before the loop-top force ends the walk, at most 16
    uint8_t need17;                  // the walk would visit a 17th seed: its record does not exist
};

// n in [seedLen, 128]; wrap: GetWrappedNextSeedToTest order (DevTables::wrap, entries 1..seedLen-1 read).
constexpr void simple_schedule(uint32_t n, uint32_t seedLen, uint32_t maxSeeds, const uint32_t *wrap,
                               SimpleSchedule &out) {
    const uint32_t nPossible = n - seedLen + 1;
    uint64_t used0 = 0, used1 = 0;   // BaseAligner::seedUsed, positions 0..63 and 64..127
    uint32_t lps = 0, nApplied = 0, seedsRcp = rcp16_of(1), next = 0, wrapCount = 0;
    out.nSteps = 0;
    out.need17 = 0;
    for (int k = 0; k < SCHED_STEPS; k++) out.lpsAfter[k] = 0;
    for (;;) {
        bool force = 2 * nApplied >= maxSeeds;
        if (!force && next >= nPossible) {
            wrapCount++;
            if (wrapCount >= seedLen) force = true;
            else {
                next = wrap[wrapCount];
                seedsRcp = rcp16_of(wrapCount + 1);
            }
        }
        if (force) break;   // (its score call leaves lps as it is: nApplied and seedsRcp are the last step's)
        while (next < nPossible && (((next < 64 ? used0 : used1) >> (next & 63)) & 1)) next++;
        if (next >= nPossible) continue;
        if (nApplied >= (uint32_t)SCHED_STEPS) { out.need17 = 1; break; }
        if (next < 64) used0 |= 1ull << next; else used1 |= 1ull << (next & 63);
        nApplied++;
        next += seedLen;
        const uint32_t v = quot_rcp16(nApplied, seedsRcp);
        if (v > lps) lps = v;
        out.lpsAfter[nApplied - 1] = (uint8_t)lps;
    }
    out.nSteps = (uint8_t)nApplied;
    for (uint32_t k = nApplied; k < (uint32_t)SCHED_STEPS; k++) out.lpsAfter[k] = (uint8_t)lps;
}

}  // namespace sgk
