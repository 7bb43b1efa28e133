// paired_state.h -- the state behind snapgpu_paired_aligner_t, shared by paired.hip (the pair
// kernels, create / free, the align calls) and paired_output.hip (CIGARs and SAM text of the
// resident pair batch).
#pragma once
#include <hip/hip_runtime.h>

#include "align_device.h"
#include "internal.h"

struct PassPool {
    char *pool = nullptr;
    uint64_t stride = 0;
    int grid = 0;
    uint32_t candCap = 0, mateCap = 0, anchorCap = 0;
};

struct PairedOutput;   // paired_output.hip

struct snapgpu_paired_aligner {
    int device = 0;
    snapgpu_paired_params_t p{};
    snapgpu_aligner_t *single = nullptr;   // the chimeric fallback's BaseAligner; owns the index upload
    sgk::KArgs X{};
    hipStream_t stream = nullptr;
    PassPool pass[3];                      // [0] passes 1 and 1b, [1] pass 3 (the reference's pools), [2] pass 2
    int grid256 = 0;                       // pass 1b (<256>) grid: at most pass[0].grid (its pools)
    int computeUnits = 0, perCU[3] = {};   // resident workgroups per CU of paired_kernel<128> / <256> / <512>: the grids' source
    uint32_t refPool = 0, maxSeedsCmd = 0;
    uint32_t *dCounter = nullptr;          // [0] pass 1 queue, [1] pass 3 queue, [2] pass-1 defer count,
                                           // [3] pass 2 queue, [4] pass-2 defer count, [5] pass 1b queue,
                                           // [6] pass-1b defer count
    uint32_t *dDefer = nullptr, *dDefer2 = nullptr;
    uint32_t *dOrder = nullptr, *dOrderW = nullptr;   // long pairs before / after pair_weight_kernel
    bool orderLong = true;                 // pass 1b longest-first (SNAPGPU_ORDER_LONG=0: input order)
    snapgpu_pair_result_t *dOut = nullptr;
    char *dB[2] = {}, *dQ[2] = {};
    uint64_t *dO[2] = {};
    uint32_t *dL[2] = {};
    uint64_t capPairs = 0, capBytes[2] = {0, 0};
    // the batch the last intersecting run left in dB / dQ / dO / dL (its reads stay there until the
    // next run): pairs and bytes per end, 0 pairs when there is none; what paired_output.hip formats
    uint64_t residentN = 0, residentBytes[2] = {0, 0};
    PairedOutput *output = nullptr;        // paired_output.hip's buffers, made by its first call
};

// ---- defined in paired_output.hip
// A new intersecting run rewrites the resident reads: the CIGARs and the text of the earlier batch
// are stale from here on (the run's copies are queued behind the output kernels on pa->stream).
void pairedOutputStale(snapgpu_paired_aligner_t *pa);
// pa->output's buffers, events and staging back to the runtime (snapgpu_paired_aligner_free).
void pairedOutputFree(snapgpu_paired_aligner_t *pa);
