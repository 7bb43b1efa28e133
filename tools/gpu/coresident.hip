// coresident.hip -- do the waves of a small kernel on a second stream run beside a resident grid
// that has align_kernel<128>'s footprint, or only when that grid's waves leave?  (DESIGN.md
// section 5, round 22.)
//
// Kernel A is the stand-in for align_kernel<128>: one-wave workgroups, 96 VGPRs, 7,552 B of static
// LDS, 20 per CU (every one resident: tools/gpu/lds_residency.hip), a compute loop bounded by an
// iteration count (a few ms), on stream 1.  That leaves a SIMD 512 - 5 * 96 = 32 VGPRs, a CU
// 10,240 B of LDS and three of eight wave slots per SIMD.  Kernel B is the stand-in for a front-stage
// kernel: 128 B of LDS, no scratch, a short bounded loop, a few thousand waves, launched on stream 2
// while A runs.  Every wave of both stores s_memrealtime at entry and exit with ordinary vector stores,
// with its HW_ID / XCC_ID.  Reported per variant: the B waves that entered before A's first wave left,
// device-wide and within each CU (B waves of a CU that entered before that CU's first A wave left).
// Variants: B at 32 and at 40 allocated VGPRs (40 cannot fit beside five 96-VGPR waves), as four-wave
// and as one-wave workgroups; and A with 22 workgroups per CU, two of them pending behind the resident
// 20, which asks whether a queue with pending workgroups holds the other queue back.  A last variant
// puts the runtime's 64 MB fill (hipMemsetAsync) in B's place and times it with events.
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/gpu/coresident tools/gpu/coresident.hip
//   timeout -k 10 120 tools/gpu/coresident > profiles/r22/coresident.json
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr uint32_t A_ITERS = 49152;      // x 8 dependent v_add_u32, 5 waves to a SIMD: about 3 ms
constexpr uint32_t B_ITERS = 512;
constexpr uint32_t B_WAVES = 4096;       // waves of B per variant

struct Stamp {
    uint64_t enter, leave;               // s_memrealtime (100 MHz)
    uint32_t hwId, xccId;                // HW_REG_HW_ID, HW_REG_XCC_ID
};

__device__ __forceinline__ uint32_t spin(uint32_t iters, uint32_t seed) {
    uint32_t r0 = threadIdx.x + seed, r1 = r0 ^ 1, r2 = r0 ^ 2, r3 = r0 ^ 3;
    const uint32_t k = (seed & 7u) + 1u;
#pragma unroll 1
    for (uint32_t it = 0; it < iters; it++) {
        asm volatile("v_add_u32 %0, %0, %4\n v_add_u32 %1, %1, %0\n v_add_u32 %2, %2, %1\n v_add_u32 %3, %3, %2\n"
                     "v_add_u32 %0, %0, %3\n v_add_u32 %1, %1, %0\n v_add_u32 %2, %2, %1\n v_add_u32 %3, %3, %2\n"
                     : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3)
                     : "s"(k));
    }
    return r0 ^ r1 ^ r2 ^ r3;
}

__device__ __forceinline__ void stamp(Stamp *out, uint32_t at, uint32_t nOut, uint64_t t0, uint64_t t1) {
    if ((threadIdx.x & 63u) == 0 && at < nOut) {
        Stamp s;
        s.enter = t0;
        s.leave = t1;
        s.hwId = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));    // HW_REG_HW_ID, 32 bits
        s.xccId = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
        out[at] = s;
    }
}

// A: align_kernel<128>'s footprint
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void body_kernel(Stamp *out, uint32_t nOut,
                                                                                            uint32_t iters, uint32_t seed,
                                                                                            uint32_t *sink) {
    __shared__ char buf[7552];
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    asm volatile("v_mov_b32 v95, 0" ::: "v95");   // the allocation reaches v95: registers cap a SIMD at 5 waves
    buf[(threadIdx.x * 113u + seed) % 7552u] = (char)threadIdx.x;
    const uint32_t x = spin(iters, seed);
    const char b = buf[x % 7552u];
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    stamp(out, blockIdx.x, nOut, t0, t1);
    if (x == 0x12345678u && b == 77) sink[0] = x;
}

// B: a front-stage kernel's footprint, VGPRS allocated registers, WAVES waves to a workgroup
template <int VGPRS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void guest_kernel(Stamp *out, uint32_t nOut, uint32_t iters, uint32_t seed,
                                                           uint32_t *sink) {
    __shared__ uint32_t tab[32];   // 128 B, as pass 0's wrap table
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    if (VGPRS == 32) asm volatile("v_mov_b32 v31, 0" ::: "v31");
    else asm volatile("v_mov_b32 v39, 0" ::: "v39");
    if (threadIdx.x < 32) tab[threadIdx.x] = threadIdx.x + seed;
    if (WAVES > 1) __syncthreads();
    const uint32_t x = spin(iters, seed) + tab[threadIdx.x & 31u];
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    stamp(out, blockIdx.x * WAVES + threadIdx.x / 64, nOut, t0, t1);
    if (x == 0x12345678u) sink[0] = x;
}

static uint32_t cu_of(const Stamp &w) {   // XCC_ID[3:0], HW_ID SE_ID[15:13], SH_ID[12], CU_ID[11:8]
    return ((w.xccId & 15u) << 8) | ((w.hwId >> 8) & 0xffu);
}

struct Ctx {
    int ncu;
    hipStream_t sA, sB;
    Stamp *dA, *dB;
    uint32_t *sink;
    uint32_t capA;
};

// one variant: A with perCU workgroups per CU on stream 1, then `guest` on stream 2
template <int VGPRS, int WAVES>
static int run(Ctx &c, int perCU, bool last) {
    const uint32_t gridA = (uint32_t)(c.ncu * perCU), gridB = B_WAVES / WAVES;
    hipFuncAttributes fa, fb;
    CHK(hipFuncGetAttributes(&fa, (const void *)body_kernel));
    CHK(hipFuncGetAttributes(&fb, (const void *)guest_kernel<VGPRS, WAVES>));
    // warm: code objects loaded, both kernels run alone
    hipLaunchKernelGGL(body_kernel, dim3(gridA), dim3(64), 0, c.sA, c.dA, c.capA, 64u, 1u, c.sink);
    CHK(hipGetLastError());
    hipLaunchKernelGGL((guest_kernel<VGPRS, WAVES>), dim3(gridB), dim3(64 * WAVES), 0, c.sB, c.dB, B_WAVES, 64u, 1u, c.sink);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipMemset(c.dA, 0, sizeof(Stamp) * c.capA));
    CHK(hipMemset(c.dB, 0, sizeof(Stamp) * B_WAVES));
    CHK(hipDeviceSynchronize());
    hipLaunchKernelGGL(body_kernel, dim3(gridA), dim3(64), 0, c.sA, c.dA, c.capA, A_ITERS, 2u, c.sink);
    CHK(hipGetLastError());
    hipLaunchKernelGGL((guest_kernel<VGPRS, WAVES>), dim3(gridB), dim3(64 * WAVES), 0, c.sB, c.dB, B_WAVES, B_ITERS, 2u, c.sink);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    std::vector<Stamp> a(gridA), b(B_WAVES);
    CHK(hipMemcpy(a.data(), c.dA, sizeof(Stamp) * gridA, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(b.data(), c.dB, sizeof(Stamp) * B_WAVES, hipMemcpyDeviceToHost));
    uint64_t aEnter = ~0ull, aFirstLeave = ~0ull, aLastLeave = 0, bEnter = ~0ull, bLastLeave = 0;
    std::map<uint32_t, uint64_t> cuFirstLeave;   // per CU: A's first exit
    for (const Stamp &w : a) {
        aEnter = std::min(aEnter, w.enter);
        aFirstLeave = std::min(aFirstLeave, w.leave);
        aLastLeave = std::max(aLastLeave, w.leave);
        auto it = cuFirstLeave.find(cu_of(w));
        if (it == cuFirstLeave.end()) cuFirstLeave[cu_of(w)] = w.leave;
        else it->second = std::min(it->second, w.leave);
    }
    uint32_t aResident = 0;
    for (const Stamp &w : a) aResident += w.enter < aFirstLeave;
    uint32_t entered = 0, finished = 0, stray = 0;
    std::map<uint32_t, uint32_t> cuCount;
    for (auto &kv : cuFirstLeave) cuCount[kv.first] = 0;
    for (const Stamp &w : b) {
        bEnter = std::min(bEnter, w.enter);
        bLastLeave = std::max(bLastLeave, w.leave);
        entered += w.enter < aFirstLeave;
        finished += w.leave < aFirstLeave;
        auto it = cuFirstLeave.find(cu_of(w));
        if (it == cuFirstLeave.end()) stray++;   // a CU that ran no A wave
        else cuCount[it->first] += w.enter < it->second;
    }
    uint32_t cuMin = ~0u, cuMax = 0, cuSum = 0;
    for (auto &kv : cuCount) { cuMin = std::min(cuMin, kv.second); cuMax = std::max(cuMax, kv.second); cuSum += kv.second; }
    printf("  {\"a_per_cu\": %d, \"a_vgprs\": %d, \"a_lds\": %zu, \"a_resident_before_first_exit\": %u, \"a_launched\": %u, "
           "\"b_vgprs_allocated\": %d, \"b_vgprs_reported\": %d, \"b_lds\": %zu, \"b_scratch\": %zu, \"b_waves_per_workgroup\": %d, "
           "\"b_waves\": %u, \"b_entered_before_a_first_exit\": %u, \"b_finished_before_a_first_exit\": %u, "
           "\"per_cu_b_entered_min\": %u, \"per_cu_b_entered_max\": %u, \"per_cu_b_entered_mean\": %.2f, \"cus_seen\": %zu, "
           "\"b_on_cu_without_a\": %u, \"b_first_enter_after_a_first_enter_us\": %.1f, \"a_first_exit_us\": %.1f, "
           "\"a_last_exit_us\": %.1f, \"b_last_exit_us\": %.1f}%s\n",
           perCU, fa.numRegs, fa.sharedSizeBytes, aResident, gridA, (VGPRS + 7) / 8 * 8, fb.numRegs, fb.sharedSizeBytes,
           fb.localSizeBytes, WAVES, B_WAVES, entered, finished, cuMin, cuMax, (double)cuSum / (double)cuCount.size(),
           cuCount.size(), stray, ((double)bEnter - (double)aEnter) / 100.0, (double)(aFirstLeave - aEnter) / 100.0,
           (double)(aLastLeave - aEnter) / 100.0, ((double)bLastLeave - (double)aEnter) / 100.0, last ? "" : ",");
    return 0;
}

// the runtime's fill in B's place: 64 MB of 0xff, as the record pre-fill of a 1M-read pass set
static int run_fill(Ctx &c) {
    const size_t bytes = 64u << 20;
    char *buf;
    hipEvent_t e0, e1, eA;
    CHK(hipMalloc(&buf, bytes));
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1)); CHK(hipEventCreate(&eA));
    CHK(hipMemsetAsync(buf, 0xff, bytes, c.sB));   // warm
    CHK(hipDeviceSynchronize());
    float alone = 0, beside = 0, body = 0;
    CHK(hipEventRecord(e0, c.sB));
    CHK(hipMemsetAsync(buf, 0xff, bytes, c.sB));
    CHK(hipEventRecord(e1, c.sB));
    CHK(hipDeviceSynchronize());
    CHK(hipEventElapsedTime(&alone, e0, e1));
    hipLaunchKernelGGL(body_kernel, dim3((uint32_t)(c.ncu * 20)), dim3(64), 0, c.sA, c.dA, c.capA, A_ITERS, 2u, c.sink);
    CHK(hipGetLastError());
    CHK(hipEventRecord(eA, c.sA));
    CHK(hipEventRecord(e0, c.sB));
    CHK(hipMemsetAsync(buf, 0xff, bytes, c.sB));
    CHK(hipEventRecord(e1, c.sB));
    CHK(hipDeviceSynchronize());
    CHK(hipEventElapsedTime(&beside, e0, e1));
    CHK(hipEventElapsedTime(&body, e0, eA));
    printf("\"fill_64MB\": {\"alone_ms\": %.3f, \"queued_behind_a_launch_ms\": %.3f, \"a_end_after_fill_queued_ms\": %.3f, "
           "\"note\": \"events on the fill's stream around hipMemsetAsync; the last figure is from the same first event to "
           "the event behind A on its stream\"}\n", alone, beside, body);
    (void)hipFree(buf);
    return 0;
}

int main() {
    hipDeviceProp_t p;
    CHK(hipGetDeviceProperties(&p, 0));
    Ctx c;
    c.ncu = p.multiProcessorCount;
    c.capA = (uint32_t)(c.ncu * 22);
    CHK(hipStreamCreateWithFlags(&c.sA, hipStreamNonBlocking));
    CHK(hipStreamCreateWithFlags(&c.sB, hipStreamNonBlocking));
    CHK(hipMalloc(&c.dA, sizeof(Stamp) * c.capA));
    CHK(hipMalloc(&c.dB, sizeof(Stamp) * B_WAVES));
    CHK(hipMalloc(&c.sink, 4));
    printf("{\"device\": \"%s\", \"cus\": %d, \"note\": \"A: one-wave workgroups, 96 VGPRs, 7,552 B LDS, a_per_cu per CU, on "
           "stream 1; B: b_waves waves of a 128-B-LDS kernel on stream 2, launched behind A from the host; entered = entry "
           "stamp (s_memrealtime) before A's first exit stamp, per_cu_* the same within each CU (XCC_ID, HW_ID)\", "
           "\"variants\": [\n", p.gcnArchName, c.ncu);
    if (run<32, 4>(c, 20, false) || run<32, 1>(c, 20, false) || run<40, 4>(c, 20, false) || run<40, 1>(c, 20, false) ||
        run<32, 4>(c, 22, false) || run<32, 1>(c, 22, true))
        return 1;
    printf("],\n");
    if (run_fill(c)) return 1;
    printf("}\n");
    return 0;
}
