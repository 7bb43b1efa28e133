// resident_grid.h -- workgroups of a persistent kernel that a CU really keeps resident.
//
// hipOccupancyMaxActiveBlocksPerMultiprocessor divides the CU's LDS by the kernel's static LDS as it
// stands; the hardware allocates LDS in units of 1,280 B (measured: tools/gpu/lds_residency.hip,
// profiles/r17/lds_residency.json -- 7,680 B: 20 one-wave workgroups per CU, 7,681..8,960 B: 18,
// 8,961 B: 16, where the API answers 20, 20 and 18).  A persistent grid sized by the API alone
// launches workgroups that wait for the first ones to leave.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>

namespace sgk {

constexpr size_t LDS_ALLOC_UNIT = 1280;

// min(the occupancy API's answer, LDS per CU / the kernel's static LDS rounded up to the allocation
// unit); `fallback` where the API gives nothing.  SNAPGPU_WAVES_PER_CU (test hook: fewer resident
// workgroups per CU than the kernel's resources allow) caps the result.
inline int resident_blocks_per_cu(const void *kernel, int blockThreads, const hipDeviceProp_t &prop, int fallback) {
    int perCU = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, blockThreads, 0) != hipSuccess || perCU <= 0)
        perCU = fallback;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kernel) == hipSuccess && fa.sharedSizeBytes > 0) {
        const size_t alloc = (fa.sharedSizeBytes + LDS_ALLOC_UNIT - 1) / LDS_ALLOC_UNIT * LDS_ALLOC_UNIT;
        const size_t fit = prop.maxSharedMemoryPerMultiProcessor / alloc;
        if (fit >= 1) perCU = (int)std::min<size_t>((size_t)perCU, fit);
    }
    (void)hipGetLastError();
    if (const char *t = getenv("SNAPGPU_WAVES_PER_CU"); t && atoi(t) > 0) perCU = std::min(perCU, atoi(t));
    return perCU;
}

}  // namespace sgk
