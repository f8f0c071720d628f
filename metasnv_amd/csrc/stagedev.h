// metasnv_amd/csrc/stagedev.h -- what the host half of every file stage's .hip file needs around its launches, once: a device buffer, the
// event pair that times the kernels, and the size of a row slab.  For the files hipcc compiles, like hiptry.h.  Every failed runtime call
// ends the stage with MSNV_EHIP through HIP_TRY; the buffers and the events go with their objects on every way out.
// The buffers are plain hipMalloc / hipFree, not the pipeline's caching allocator (devmem.hip): what hipMemGetInfo reports to slab_rows, and
// what the process holds between two calls, is then the stage's own doing.
#pragma once

#include <algorithm>

#include "hiptry.h"

#define MSNV_TRY(expr)                       \
    do {                                     \
        if (int rc_ = (expr)) return rc_;    \
    } while (0)

namespace msnv {

struct Buf {
    void *p = nullptr;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { if (p) (void)hipFree(p); }
    template <class T> T *as() const { return (T *)p; }
    int alloc(size_t bytes) {                                          // never fewer than 16 bytes: an empty table still has an address
        HIP_TRY(hipMalloc(&p, std::max<size_t>(bytes, 16)));
        return MSNV_OK;
    }
    int upload(const void *src, size_t bytes, hipStream_t st) {
        MSNV_TRY(alloc(bytes));
        if (bytes) HIP_TRY(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st));
        return MSNV_OK;
    }
};

// The kernels of a stage between two events; ms adds up over begin / end pairs.  end is stop + wait: a stage that queues its downloads behind the
// kernels calls stop, queues them, then wait -- one wait for both, and the events bracket the kernels alone.
struct KernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0;
    KernelTimer() = default;
    KernelTimer(const KernelTimer &) = delete;
    KernelTimer &operator=(const KernelTimer &) = delete;
    ~KernelTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int begin(hipStream_t st) {
        if (!e0) HIP_TRY(hipEventCreate(&e0));
        if (!e1) HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        return MSNV_OK;
    }
    int stop(hipStream_t st) {                                         // behind the last launch
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e1, st));
        return MSNV_OK;
    }
    int wait(hipStream_t st) {
        HIP_TRY(hipStreamSynchronize(st));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e0, e1));
        ms += t;
        return MSNV_OK;
    }
    int end(hipStream_t st) { MSNV_TRY(stop(st)); return wait(st); }
};

// Rows per slab of a table that a stage walks in row slabs: what `fraction` of the free device memory holds at row_bytes each, at most the
// table's n_rows (one row for an empty table), the stage's own row_cap, and MSNV_STAGE_SLAB_ROWS (knobs.h; read here and nowhere else).
inline int slab_rows(uint64_t n_rows, uint64_t row_bytes, double fraction, uint64_t row_cap, const char *what, uint64_t *rows) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *rows = std::min(std::min(std::max<uint64_t>(n_rows, 1), (uint64_t)(free_b * fraction) / row_bytes), row_cap);
    if (*rows == 0) return fail(MSNV_ENOMEM, "%s: %llu bytes of device memory left, one row takes %llu", what, (unsigned long long)free_b, (unsigned long long)row_bytes);
    if (const uint64_t knob_rows = knob::stage_slab_rows()) *rows = std::min(*rows, knob_rows);
    return MSNV_OK;
}

}  // namespace msnv
