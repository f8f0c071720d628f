// metasnv_amd/csrc/snvfreq_k.hip -- the counts behind subpopr's SNV-frequency plots (src/subpopr/R/snvFreqPlot.R:1-113 and
// computeSnvFreqStats.R:31-46; the host half is snvfreq.cpp).
//
//   msnv_freq_curves_k   per sample column: how many covered cells are <= k and how many are >= 100 - k for k = 0..49, how many are covered,
//                        and how many lie outside a strict band (x < lo | x > hi)
// A covered cell x in [0, 100] belongs to at most one class: x <= k iff ceil(x) <= k, so its low class is ceil(x) when that is <= 49; x >= 100 - k
// iff 100 - floor(x) <= k, so its high class is 100 - floor(x) when that is <= 49; a cell in (49, 51) has neither.  ceil, floor and the
// difference are exact in fp64.  The kernel counts the classes; dev_freq_curves takes the running sums over k on the host (102 integers a sample).
//
// Access pattern of msnv_freq_bands_k (cluster_k.hip): a thread per sample column, the lanes of a wavefront read consecutive columns of one row, a
// block walks FREQ_CURVE_ROWS rows.  A block is ONE wavefront of FREQ_CURVE_LANES = 64.  The 100 class counters of a thread are u32 in LDS, laid
// out [class][lane]: lane l's word is always in bank l mod 32 whatever its class, so the lanes of a wavefront never share a bank, and a counter
// belongs to one thread, so no atomics and no barrier.  100 x 64 x 4 = 25 600 bytes of static LDS: under the 48 KiB limit (no opt-in) and six blocks a
// CU.  u32 cannot overflow: a block adds at most FREQ_CURVE_ROWS to a counter.  The covered and the strict count stay in registers.  Only the flush
// touches global memory: one u64 atomicAdd per non-zero counter, into counters laid out [class][sample] so that the lanes of a flush are
// neighbours.  Integers: the result does not depend on the grid, the slab cuts or the order of the flushes.
// A cell outside [0, 100] (infinities included) is not counted and raises the flag word: the caller refuses the table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

namespace msnv {

constexpr uint32_t FREQ_CURVE_CLASSES = 100, FREQ_CURVE_UNROLL = 8;

// cnt[class][lane]; the class of a cell that has one
__device__ __forceinline__ void freq_curve_cell(double x, double lo, double hi, uint32_t *cnt, uint32_t lane, uint32_t &covered, uint32_t &strict, uint32_t &outside) {
    if (x != x) return;
    if (!(x >= 0.0 && x <= 100.0)) { outside = 1; return; }
    ++covered;
    strict += (x < lo || x > hi) ? 1 : 0;
    const uint32_t low = (uint32_t)ceil(x), high = 100u - (uint32_t)floor(x);      // both 0..100
    if (low < 50) cnt[low * FREQ_CURVE_LANES + lane] += 1;
    else if (high < 50) cnt[(50 + high) * FREQ_CURVE_LANES + lane] += 1;
}

// counts[102][S]: [c] cells of low class c, [50 + c] cells of high class c, [100] covered cells, [101] cells outside the strict band
__global__ void __launch_bounds__(FREQ_CURVE_LANES) msnv_freq_curves_k(const double *__restrict__ rows, unsigned long long n_pos, uint32_t S, double lo, double hi,
                                                                      unsigned long long *__restrict__ counts, uint32_t *__restrict__ flag) {
    __shared__ uint32_t cnt[FREQ_CURVE_CLASSES * FREQ_CURVE_LANES];
    const uint32_t lane = threadIdx.x, s = blockIdx.x * FREQ_CURVE_LANES + lane;
    if (s >= S) return;                                                // no barrier below: a thread's counters are its own
    for (uint32_t c = 0; c < FREQ_CURVE_CLASSES; ++c) cnt[c * FREQ_CURVE_LANES + lane] = 0;
    const unsigned long long p0 = (unsigned long long)blockIdx.y * FREQ_CURVE_ROWS, p1 = p0 + FREQ_CURVE_ROWS < n_pos ? p0 + FREQ_CURVE_ROWS : n_pos;
    uint32_t covered = 0, strict = 0, outside = 0;
    const double *col = rows + s;
    unsigned long long p = p0;
    for (; p + FREQ_CURVE_UNROLL <= p1; p += FREQ_CURVE_UNROLL) {      // the loads of a round are in flight together
        double x[FREQ_CURVE_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < FREQ_CURVE_UNROLL; ++u) x[u] = col[(p + u) * S];
#pragma unroll
        for (uint32_t u = 0; u < FREQ_CURVE_UNROLL; ++u) freq_curve_cell(x[u], lo, hi, cnt, lane, covered, strict, outside);
    }
    for (; p < p1; ++p) freq_curve_cell(col[p * S], lo, hi, cnt, lane, covered, strict, outside);
    for (uint32_t c = 0; c < FREQ_CURVE_CLASSES; ++c)
        if (const uint32_t v = cnt[c * FREQ_CURVE_LANES + lane]) atomicAdd(&counts[(size_t)c * S + s], (unsigned long long)v);
    if (covered) atomicAdd(&counts[(size_t)100 * S + s], (unsigned long long)covered);
    if (strict) atomicAdd(&counts[(size_t)101 * S + s], (unsigned long long)strict);
    if (outside) atomicOr(flag, 1u);
}

// counts[sample][102] as include/msnv.h lays them out; *outside = 1 when a cell was neither NaN nor within [0, 100] (the counts then leave it out)
int dev_freq_curves(const double *rows, uint64_t n_pos, uint32_t S, double lo, double hi, void *stream_, uint64_t *counts, uint32_t *outside, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    const size_t cnt_bytes = (size_t)S * 102 * 8;
    Buf d_rows, d_cnt, d_flag;
    MSNV_TRY(d_cnt.alloc(cnt_bytes));
    MSNV_TRY(d_flag.alloc(4));
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, cnt_bytes, st));
    HIP_TRY(hipMemsetAsync(d_flag.p, 0, 4, st));
    // position slabs that fit the device and the grid's second dimension
    const uint64_t row_bytes = (uint64_t)S * 8;
    uint64_t chunk = 0;
    MSNV_TRY(slab_rows(n_pos, row_bytes, 0.5, (uint64_t)FREQ_CURVE_ROWS * 65535, "SNV frequency curves", &chunk));
    MSNV_TRY(d_rows.alloc(chunk * row_bytes));
    KernelTimer tm;
    for (uint64_t p0 = 0; p0 < n_pos; p0 += chunk) {
        const uint64_t np = std::min(chunk, n_pos - p0);
        HIP_TRY(hipMemcpyAsync(d_rows.p, rows + p0 * S, np * row_bytes, hipMemcpyHostToDevice, st));
        MSNV_TRY(tm.begin(st));
        hipLaunchKernelGGL(msnv_freq_curves_k, dim3((S + FREQ_CURVE_LANES - 1) / FREQ_CURVE_LANES, (uint32_t)((np + FREQ_CURVE_ROWS - 1) / FREQ_CURVE_ROWS)),
                           dim3(FREQ_CURVE_LANES), 0, st, d_rows.as<double>(), (unsigned long long)np, S, lo, hi, d_cnt.as<unsigned long long>(), d_flag.as<uint32_t>());
        MSNV_TRY(tm.end(st));
    }
    std::vector<uint64_t> by_class((size_t)S * 102);
    HIP_TRY(hipMemcpyAsync(by_class.data(), d_cnt.p, cnt_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(outside, d_flag.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t s = 0; s < S; ++s) {
        uint64_t *out = counts + (size_t)s * 102, low = 0, high = 0;
        for (uint32_t k = 0; k < 50; ++k) {
            out[k] = low += by_class[(size_t)k * S + s];
            out[50 + k] = high += by_class[(size_t)(50 + k) * S + s];
        }
        out[100] = by_class[(size_t)100 * S + s];
        out[101] = by_class[(size_t)101 * S + s];
    }
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
