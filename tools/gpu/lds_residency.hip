// lds_residency.hip -- how many one-wave workgroups of a given static LDS size a gfx950 CU keeps
// resident at once.
//
// align_kernel<128> launches 20 one-wave workgroups per CU (what the occupancy API reports for its
// 96 VGPRs and 8,096 B of LDS), yet its wave stamps show about a tenth of them entering only when the
// first ones leave.  Neither the compiler's occupancy remark nor the occupancy API models the LDS
// allocation granule.  This probe measures it: for each static LDS size it launches 20 x CU-count
// one-wave workgroups at 96 VGPRs; every wave stamps s_memrealtime at entry, runs a compute loop
// bounded by an iteration count (a few hundred microseconds), stamps again and exits.  Reported per
// size: the waves that entered before the first one left (device-wide, and per CU by HW_ID / XCC_ID:
// waves of a CU that entered before that CU's first wave left).
//
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/lds_residency tools/gpu/lds_residency.hip
//   timeout -k 10 60 /tmp/lds_residency > profiles/r17/lds_residency.json
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int WAVES_PER_CU = 20;
constexpr uint32_t ITERS = 4096;         // x 8 dependent v_add_u32 per iteration, 5 waves to a SIMD

struct Stamp {
    uint64_t enter, leave;               // s_memrealtime (100 MHz)
    uint32_t hwId, xccId;                // HW_REG_HW_ID, HW_REG_XCC_ID
};

template <int LDS_BYTES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void residency_kernel(Stamp *out, uint32_t nOut,
                                                                                                 uint32_t iters, uint32_t seed,
                                                                                                 uint32_t *sink) {
    __shared__ char buf[LDS_BYTES];
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    const uint32_t lane = threadIdx.x;
    // 96 VGPRs, as align_kernel<128>: the allocation reaches v95, so registers cap a SIMD at 5 waves
    asm volatile("v_mov_b32 v95, 0" ::: "v95");
    buf[(lane * 113u + seed) % (uint32_t)LDS_BYTES] = (char)lane;
    uint32_t r0 = lane + seed, r1 = r0 ^ 1, r2 = r0 ^ 2, r3 = r0 ^ 3;
    const uint32_t k = (seed & 7u) + 1u;
#pragma unroll 1
    for (uint32_t it = 0; it < iters; it++) {
        asm volatile("v_add_u32 %0, %0, %4\n v_add_u32 %1, %1, %0\n v_add_u32 %2, %2, %1\n v_add_u32 %3, %3, %2\n"
                     "v_add_u32 %0, %0, %3\n v_add_u32 %1, %1, %0\n v_add_u32 %2, %2, %1\n v_add_u32 %3, %3, %2\n"
                     : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3)
                     : "s"(k));
    }
    const uint32_t x = r0 ^ r1 ^ r2 ^ r3;
    const char b = buf[x % (uint32_t)LDS_BYTES];
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0 && blockIdx.x < nOut) {
        Stamp s;
        s.enter = t0;
        s.leave = t1;
        s.hwId = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));    // HW_REG_HW_ID, 32 bits
        s.xccId = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
        out[blockIdx.x] = s;
    }
    if (x == 0x12345678u && b == 77) sink[0] = x;
}

template <int LDS_BYTES>
static int run(int ncu, bool last) {
    const uint32_t grid = (uint32_t)(ncu * WAVES_PER_CU);
    Stamp *d;
    uint32_t *ds;
    CHK(hipMalloc(&d, sizeof(Stamp) * grid));
    CHK(hipMalloc(&ds, 4));
    hipFuncAttributes fa;
    CHK(hipFuncGetAttributes(&fa, (const void *)residency_kernel<LDS_BYTES>));
    int api = 0;
    CHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, (const void *)residency_kernel<LDS_BYTES>, 64, 0));
    hipLaunchKernelGGL(residency_kernel<LDS_BYTES>, dim3(grid), dim3(64), 0, 0, d, grid, 64u, 1u, ds);   // warm
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipMemset(d, 0, sizeof(Stamp) * grid));
    hipLaunchKernelGGL(residency_kernel<LDS_BYTES>, dim3(grid), dim3(64), 0, 0, d, grid, ITERS, 2u, ds);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    std::vector<Stamp> s(grid);
    CHK(hipMemcpy(s.data(), d, sizeof(Stamp) * grid, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    (void)hipFree(ds);
    uint64_t firstEnter = ~0ull, firstLeave = ~0ull, lastLeave = 0;
    for (const Stamp &w : s) {
        firstEnter = std::min(firstEnter, w.enter);
        firstLeave = std::min(firstLeave, w.leave);
        lastLeave = std::max(lastLeave, w.leave);
    }
    uint32_t before = 0;
    for (const Stamp &w : s) before += w.enter < firstLeave;
    // per CU: XCC_ID[3:0], HW_ID SE_ID[15:13], SH_ID[12], CU_ID[11:8]
    std::map<uint32_t, std::vector<const Stamp *>> cus;
    for (const Stamp &w : s) cus[((w.xccId & 15u) << 8) | ((w.hwId >> 8) & 0xffu)].push_back(&w);
    uint32_t cuMin = ~0u, cuMax = 0, cuSum = 0, wavesMin = ~0u, wavesMax = 0;
    for (auto &kv : cus) {
        uint64_t fl = ~0ull;
        for (const Stamp *w : kv.second) fl = std::min(fl, w->leave);
        uint32_t c = 0;
        for (const Stamp *w : kv.second) c += w->enter < fl;
        cuMin = std::min(cuMin, c); cuMax = std::max(cuMax, c); cuSum += c;
        wavesMin = std::min<uint32_t>(wavesMin, (uint32_t)kv.second.size());
        wavesMax = std::max<uint32_t>(wavesMax, (uint32_t)kv.second.size());
    }
    printf("  {\"lds_bytes\": %d, \"static_lds_reported\": %zu, \"vgprs\": %d, \"api_blocks_per_cu\": %d, \"launched\": %u, "
           "\"entered_before_first_exit\": %u, \"per_cu_device_wide\": %.2f, \"cus_seen\": %zu, "
           "\"per_cu_resident_min\": %u, \"per_cu_resident_max\": %u, \"per_cu_resident_mean\": %.2f, "
           "\"waves_per_cu_min\": %u, \"waves_per_cu_max\": %u, \"first_wave_us\": %.1f, \"launch_us\": %.1f}%s\n",
           LDS_BYTES, fa.sharedSizeBytes, fa.numRegs, api, grid, before, (double)before / ncu, cus.size(), cuMin, cuMax,
           (double)cuSum / (double)cus.size(), wavesMin, wavesMax, (double)(firstLeave - firstEnter) / 100.0,
           (double)(lastLeave - firstEnter) / 100.0, last ? "" : ",");
    return 0;
}

int main() {
    hipDeviceProp_t p;
    CHK(hipGetDeviceProperties(&p, 0));
    const int ncu = p.multiProcessorCount;
    printf("{\"device\": \"%s\", \"cus\": %d, \"lds_per_cu\": %zu, \"waves_launched_per_cu\": %d, \"note\": \"one-wave workgroups "
           "at 96 VGPRs; entered_before_first_exit = waves whose entry stamp (s_memrealtime) precedes the first exit stamp; "
           "per_cu_resident_* = the same within each CU (XCC_ID, HW_ID)\", \"sizes\": [\n",
           p.gcnArchName, ncu, (size_t)p.maxSharedMemoryPerMultiProcessor, WAVES_PER_CU);
    // the unit's edges (7,680 | 7,681 and 8,960 | 8,961), 8,192 = 160 KB / 20, and align_kernel<128>'s sizes:
    // 8,096 B before round 17, 7,552 B (16 LV rows) and 7,936 B (30 rows) since
    if (run<7552>(ncu, false) || run<7680>(ncu, false) || run<7681>(ncu, false) || run<7936>(ncu, false) ||
        run<8096>(ncu, false) || run<8192>(ncu, false) || run<8960>(ncu, false) || run<8961>(ncu, true))
        return 1;
    printf("]}\n");
    return 0;
}
