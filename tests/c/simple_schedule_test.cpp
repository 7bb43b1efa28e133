// The walk schedule of the simple pass (snap-rnaseq_amd/csrc/simple_schedule.h) against a transcription
// of simple_one's seed loop (simple_align.h) run on an all-ACGT read whose seeds never hit: with no score
// limit (the loop-top force ends the walk) and with every score limit 0 .. 17 (the walk ends at the first
// step whose lowestPossibleScore passes it).  Every n in [seedLen, 128] for seedLen 16, 20, 23, 31 and
// maxSeeds = (int)(seedCoverage * n / seedLen) at the default coverage 4, or the fixed 8, 25, 40.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "simple_schedule.h"

namespace {

// SeedSequencer.h's wrap order as the library's tables hold it (aligner.hip kWrap; seedLen 31: none)
const uint8_t kWrap16[25] = {0, 8, 4, 12, 2, 6, 10, 14, 1, 3, 5, 7, 9, 11, 13, 15};
const uint8_t kWrap20[25] = {0, 10, 5, 15, 2, 7, 12, 17, 3, 9, 11, 13, 19, 1, 4, 6, 8, 14, 18, 16};
const uint8_t kWrap23[25] = {0, 12, 6, 17, 3, 9, 20, 14, 1, 4, 7, 10, 15, 18, 21, 4, 2, 5, 11, 16, 19, 22, 8};

struct Walk {
    int nVisited;          // seeds looked up
    int lpsB[64], lpsA[64];   // lps when step k's hits would be inserted / after its score call
    bool need17;           // the loop asked for record 16
    bool byLimit;          // ended by lps > limit (else by the loop-top force)
};

// simple_one's loop, lines "for (;;)" .. "if (forced) break", with no hit and no element
Walk walk(uint32_t n, uint32_t seedLen, uint32_t maxSeeds, const uint32_t *wrapT, uint32_t scoreLimit) {
    Walk w;
    memset(&w, 0, sizeof(w));
    const uint32_t nPossible = n - seedLen + 1;
    bool used[128] = {};
    uint32_t lps = 0, nApplied = 0, mostSeeds = 1, next = 0, wrapCount = 0, pfIdx = 0;
    for (int guard = 0; guard < 100000; guard++) {
        bool force = 2 * nApplied >= maxSeeds;
        if (!force && next >= nPossible) {
            wrapCount++;
            if (wrapCount >= seedLen) force = true;
            else {
                next = wrapT[wrapCount];
                mostSeeds = wrapCount + 1;
            }
        }
        if (!force) {
            while (next < nPossible && used[next]) next++;
            if (next >= nPossible) continue;
            used[next] = true;
            if (pfIdx >= 16) { w.need17 = true; return w; }
            w.lpsB[pfIdx] = (int)lps;
            pfIdx++;
            nApplied++;
            next += seedLen;
        }
        const uint32_t v = nApplied / mostSeeds;   // (the kernel: quot_rcp16, small_div_test.cpp)
        if (v > lps) lps = v;
        if (!force) { w.lpsA[pfIdx - 1] = (int)lps; w.nVisited = (int)pfIdx; }
        if (force) return w;
        if (lps > scoreLimit) { w.byLimit = true; return w; }
    }
    w.nVisited = -1;
    return w;
}

}  // namespace

int main() {
    unsigned long cases = 0, bad = 0;
    const uint32_t seedLens[4] = {16, 20, 23, 31};
    for (uint32_t L : seedLens) {
        uint32_t wrapT[32] = {};
        const uint8_t *src = L == 16 ? kWrap16 : L == 20 ? kWrap20 : L == 23 ? kWrap23 : nullptr;
        for (int i = 0; src && i < 25; i++) wrapT[i] = src[i];
        for (uint32_t n = L; n <= 128; n++) {
            const uint32_t ms[4] = {(uint32_t)(int)(4.0 * (double)n / (double)L), 8, 25, 40};
            for (uint32_t maxSeeds : ms) {
                sgk::SimpleSchedule s;
                sgk::simple_schedule(n, L, maxSeeds, wrapT, s);
                const Walk f = walk(n, L, maxSeeds, wrapT, 0xffffffffu);
                cases++;
                bool ok = f.nVisited >= 0 && !f.byLimit && (int)s.nSteps == (f.need17 ? 16 : f.nVisited) &&
                          (s.need17 != 0) == f.need17;
                for (int k = 0; ok && k < s.nSteps; k++) {
                    const int before = k ? s.lpsAfter[k - 1] : 0;
                    ok = before == f.lpsB[k] && (int)s.lpsAfter[k] == f.lpsA[k];
                }
                if (!ok && bad++ < 10)
                    printf("n %u L %u maxSeeds %u: nSteps %d/%d need17 %d/%d\n", n, L, maxSeeds, s.nSteps, f.nVisited,
                           s.need17, (int)f.need17);
                for (uint32_t lim = 0; lim <= 17; lim++) {
                    const Walk g = walk(n, L, maxSeeds, wrapT, lim);
                    cases++;
                    // the schedule's answer: the first step whose lps passes the limit ends the walk after
                    // its lookup; without one the force does (or record 16 is asked for)
                    int e = -1;
                    for (int k = 0; k < s.nSteps && e < 0; k++)
                        if (s.lpsAfter[k] > lim) e = k;
                    const bool ok2 = e >= 0 ? (g.byLimit && !g.need17 && g.nVisited == e + 1)
                                            : (!g.byLimit && g.need17 == (s.need17 != 0) &&
                                               (g.need17 || g.nVisited == (int)s.nSteps));
                    if (!ok2 && bad++ < 10)
                        printf("n %u L %u maxSeeds %u limit %u: schedule ends at %d, loop visited %d (byLimit %d need17 %d)\n",
                               n, L, maxSeeds, lim, e, g.nVisited, (int)g.byLimit, (int)g.need17);
                }
            }
        }
    }
    printf("%lu cases, %lu mismatches\n", cases, bad);
    return bad != 0;
}
