// large_copy.h -- copies of large pageable host buffers to and from the device through two
// pinned staging buffers: host threads fill (or drain) one while the DMA engine works on the
// other (the index tables, up to tens of GB for a human-sized genome; a plain pageable
// hipMemcpy runs far below PCIe speed).  Shared by aligner.hip and index_build.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "internal.h"

namespace snapgpu {

// toDevice: dev <- host, else host <- dev.  The stream is idle when this returns.
inline int copyLarge(hipStream_t s, void *dev, void *host, uint64_t bytes, bool toDevice) {
    const char *what = toDevice ? "uploadLarge: " : "downloadLarge: ";
    if (bytes == 0) return SNAPGPU_OK;
    int rc = SNAPGPU_OK;
    auto fail = [&](hipError_t e) {
        setError(std::string(what) + hipGetErrorString(e));
        rc = SNAPGPU_EDEVICE;
    };
    hipError_t e;
    if (bytes < (64ull << 20)) {
        e = toDevice ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s)
                     : hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { fail(e); return rc; }
        if ((e = hipStreamSynchronize(s)) != hipSuccess) fail(e);
        return rc;
    }
    const uint64_t CH = 256ull << 20;
    void *stg[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int i = 0; i < 2 && rc == SNAPGPU_OK; i++) {
        if ((e = hipHostMalloc(&stg[i], CH, hipHostMallocDefault)) != hipSuccess) fail(e);
        else if ((e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) fail(e);
    }
    const unsigned nt = hostThreads(8);
    // the host side of chunk k: pageable <-> staging buffer k & 1, in nt slices
    auto hostCopy = [&](uint64_t k) {
        const uint64_t off = k * CH, len = std::min(CH, bytes - off);
        char *st = (char *)stg[k & 1], *h = (char *)host + off;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++)
            th.emplace_back([=] {
                const uint64_t a0 = len * t / nt, a1 = len * (t + 1) / nt;
                if (toDevice) memcpy(st + a0, h + a0, a1 - a0);
                else memcpy(h + a0, st + a0, a1 - a0);
            });
        for (auto &x : th) x.join();
    };
    const uint64_t nChunks = (bytes + CH - 1) / CH;
    if (toDevice) {
        for (uint64_t k = 0; k < nChunks && rc == SNAPGPU_OK; k++) {
            const int b = (int)(k & 1);
            const uint64_t off = k * CH, len = std::min(CH, bytes - off);
            if (k >= 2 && (e = hipEventSynchronize(ev[b])) != hipSuccess) { fail(e); break; }
            hostCopy(k);
            if ((e = hipMemcpyAsync((char *)dev + off, stg[b], len, hipMemcpyHostToDevice, s)) != hipSuccess) { fail(e); break; }
            if ((e = hipEventRecord(ev[b], s)) != hipSuccess) { fail(e); break; }
        }
    } else {
        // chunk k's DMA is queued before chunk k - 1 is drained on the host
        for (uint64_t k = 0; k <= nChunks && rc == SNAPGPU_OK; k++) {
            if (k < nChunks) {
                const int b = (int)(k & 1);
                const uint64_t off = k * CH, len = std::min(CH, bytes - off);
                if ((e = hipMemcpyAsync(stg[b], (const char *)dev + off, len, hipMemcpyDeviceToHost, s)) != hipSuccess) { fail(e); break; }
                if ((e = hipEventRecord(ev[b], s)) != hipSuccess) { fail(e); break; }
            }
            if (k >= 1) {
                if ((e = hipEventSynchronize(ev[(k - 1) & 1])) != hipSuccess) { fail(e); break; }
                hostCopy(k - 1);
            }
        }
    }
    if ((e = hipStreamSynchronize(s)) != hipSuccess && rc == SNAPGPU_OK) fail(e);
    for (int i = 0; i < 2; i++) {
        if (stg[i]) hipHostFree(stg[i]);
        if (ev[i]) hipEventDestroy(ev[i]);
    }
    return rc;
}

inline int uploadLarge(hipStream_t s, void *dst, const void *src, uint64_t bytes) {
    return copyLarge(s, dst, const_cast<void *>(src), bytes, true);
}
inline int downloadLarge(hipStream_t s, void *dst, const void *src, uint64_t bytes) {
    return copyLarge(s, const_cast<void *>(src), dst, bytes, false);
}

}  // namespace snapgpu
