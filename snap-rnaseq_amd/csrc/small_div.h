// small_div.h -- exact quotient of a small dividend by a small divisor without a division:
// a / d == (a * rcp16_of(d)) >> 16 for 0 <= a <= SDIV_MAX_A and 1 <= d <= SDIV_MAX_D.
//
// The seed loop's "seeds applied per base" bound (BaseAligner.cpp:993-996: nSeedsApplied /
// mostSeedsContainingAnyParticularBase) is taken once per score call on wave-uniform values.  The
// GPU has no scalar division: `/` there is ~25 VALU instructions and a trip back to an SGPR.  The
// divisor changes only when the seed sequence wraps, so its reciprocal is read from a host-built
// table (DevTables::rcp16) at that point and the quotient is one scalar multiply and a shift.
//
// Exactness: m = ceil(2^16 / d) = (2^16 + e) / d with 0 <= e < d, so a * m / 2^16 = a / d + a * e /
// (d * 2^16).  The floor is a / d's while a * e < 2^16 (the fraction added stays below 1 / d):
// 512 * 31 < 2^16.  The product a * m <= 512 * 65536 fits 32 bits.  (Plain C++: host and device;
// tests/c/small_div_test.cpp compares every pair with `/`.)
#pragma once
#include <stdint.h>

namespace sgk {

constexpr uint32_t SDIV_MAX_A = 512;   // dividends: seeds applied <= seed positions of a read <= 512 bases
constexpr uint32_t SDIV_MAX_D = 32;    // divisors: wrapCount + 1 <= seedLen <= 32

constexpr uint32_t rcp16_of(uint32_t d) { return (65536u + d - 1u) / d; }
constexpr uint32_t quot_rcp16(uint32_t a, uint32_t rcp) { return (a * rcp) >> 16; }

constexpr bool sdiv_exact() {
    for (uint32_t d = 1; d <= SDIV_MAX_D; d++)
        for (uint32_t a = 0; a <= SDIV_MAX_A; a++)
            if (quot_rcp16(a, rcp16_of(d)) != a / d) return false;
    return true;
}
static_assert(sdiv_exact(), "quot_rcp16 must equal / over the whole range");

}  // namespace sgk
