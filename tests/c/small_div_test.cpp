// The seed loop's division-free quotient (snap-rnaseq_amd/csrc/small_div.h) against `/`, for every
// dividend 0..512 and divisor 1..32: the range of nSeedsApplied / mostSeedsContainingAnyParticularBase.
#include <cstdint>
#include <cstdio>

#include "small_div.h"

int main() {
    unsigned bad = 0, n = 0;
    for (uint32_t d = 1; d <= 32; d++) {
        const uint32_t rcp = sgk::rcp16_of(d);
        for (uint32_t a = 0; a <= 512; a++, n++) {
            const uint32_t q = sgk::quot_rcp16(a, rcp);
            if (q != a / d) {
                if (bad++ < 10) printf("%u / %u: got %u, want %u (rcp %u)\n", a, d, q, a / d, rcp);
            }
        }
    }
    static_assert(sgk::SDIV_MAX_A == 512 && sgk::SDIV_MAX_D == 32, "the table's range");
    // the product stays inside 32 bits at the largest dividend and reciprocal
    if ((uint64_t)512 * sgk::rcp16_of(1) > 0xffffffffull) { printf("product overflows\n"); bad++; }
    printf("%u pairs, %u mismatches\n", n, bad);
    return bad != 0;
}
