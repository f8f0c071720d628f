// metasnv_amd/csrc/profile_k.hip -- per-sample statistics of a cluster's genotyping SNVs on the device (src/subpopr/R/writeSubpopsForAllSamples.R:
// 72-101; the host side is profile.cpp, the rule is stated in include/msnv.h).
//
//   msnv_profile_columns_k   per column of a row-major fp64 matrix [G x S] (NaN = no coverage, rows flipped to 100 - x where flip[g] is set): the
//                            count of called cells, of cells > 0, >= 5, == 0 and == 100, and the two middle order statistics of the called
//                            cells (0-based ranks (n - 1) / 2 and n / 2), as the exact fp64 values that occur in the column
//
// Radix selection on the cells' bit patterns: a cell in [0, 100] is a non-negative double and orders as its 64-bit pattern (-0.0 is read as
// +0.0), so eight passes over the column, one per byte from the top, each narrow the wanted ranks to one of 256 bins.  Nothing is sorted, moved
// or written back; every pass re-reads the matrix and the flip is applied as a cell is read.
// A workgroup owns PROF_COLS = 16 adjacent columns and all their rows.  A lane is (column, sub-row): 16 lanes read 128 adjacent bytes of one row,
// a wavefront four rows, the workgroup's 16 wavefronts 64 rows per step and four steps in flight per lane.  The histograms are hist[bin][column]
// in LDS, filled with LDS atomics: the lanes of one instruction that share a bin still address 16 different words, so the bin that holds nearly
// every cell of a real table (exact 0, exact 100) serialises at most the four sub-rows of a wavefront, never the columns.  n differs per column:
// the ranks are per column, taken from the pass-0 count.
// Both ranks are narrowed at once.  They share a prefix until a pass puts them into different bins (they are neighbours in the order, so the low
// one is then the largest cell of its prefix and the high one the smallest of its own); from there the second histogram follows the high rank.
// The grid is ceil(S / 16) workgroups: 256 at 4096 samples, one at 6 samples, whose 16 wavefronts then split the rows between them.
// The matrix goes up in bands of columns (a 2-D copy: a column needs all of its rows resident), as wide as half of the free memory allows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

namespace msnv {

namespace {

constexpr uint32_t PROF_BINS = 256, PROF_UNROLL = 4, PROF_ROWS_PER_STEP = PROF_WAVES * 64 / PROF_COLS;

// the key of a cell: called = neither NaN nor outside [0, 100]
__device__ inline unsigned long long prof_key(double x, bool flipped, bool &called, bool &outside) {
    if (flipped) x = 100.0 - x;                                        // NaN stays NaN
    const bool nan = x != x;
    outside = !nan && !(x >= 0.0 && x <= 100.0);
    called = !nan && !outside;
    const unsigned long long k = (unsigned long long)__double_as_longlong(x);
    return k == 0x8000000000000000ull ? 0ull : k;                      // -0.0 -> +0.0
}

}  // namespace

__global__ void __launch_bounds__(PROF_WAVES * 64) msnv_profile_columns_k(const double *__restrict__ rows, uint32_t n_rows, uint32_t ld, uint32_t n_cols,
                                                                          const uint8_t *__restrict__ flip, uint32_t *__restrict__ counts, double *__restrict__ mids,
                                                                          uint32_t *__restrict__ bad_flag) {
    __shared__ uint32_t hist[2][PROF_BINS * PROF_COLS];                // [which rank][bin][column]
    __shared__ uint32_t cnt[5][PROF_COLS];                             // called, > 0, >= 5, == 0, == 100
    __shared__ unsigned long long pfx[2][PROF_COLS];                   // the bits found so far of the low and the high rank's value
    __shared__ uint32_t rank[2][PROF_COLS];                            // their ranks among the cells that share the prefix
    __shared__ uint32_t split[PROF_COLS];                              // 1 once the two prefixes differ
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & (PROF_COLS - 1), sub = lane / PROF_COLS;
    const uint32_t c = blockIdx.x * PROF_COLS + col;
    const bool active = c < n_cols;
    const uint32_t slot = wave * (64 / PROF_COLS) + sub;               // 0 .. PROF_ROWS_PER_STEP - 1
    if (tid < 5 * PROF_COLS) cnt[tid / PROF_COLS][tid % PROF_COLS] = 0;
    if (tid < PROF_COLS) { pfx[0][tid] = pfx[1][tid] = 0; rank[0][tid] = rank[1][tid] = 0; split[tid] = 0; }

    for (uint32_t pass = 0; pass < 8; ++pass) {
        const uint32_t shift = 56 - 8 * pass;
        for (uint32_t i = tid; i < 2 * PROF_BINS * PROF_COLS; i += PROF_WAVES * 64) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned long long want0 = pfx[0][col] >> shift >> 8, want1 = pfx[1][col] >> shift >> 8;       // pass 0: both 0, as every key's
        const bool two = split[col] != 0;
        uint32_t n_called = 0, n_gt0 = 0, n_ge5 = 0, n_eq0 = 0, n_eq100 = 0;
        bool any_outside = false;
        for (uint32_t g0 = slot; g0 < n_rows; g0 += PROF_ROWS_PER_STEP * PROF_UNROLL) {
            double x[PROF_UNROLL];
            bool f[PROF_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < PROF_UNROLL; ++u) {
                const uint32_t g = g0 + u * PROF_ROWS_PER_STEP;
                const bool in = active && g < n_rows;
                x[u] = in ? rows[(size_t)g * ld + c] : __longlong_as_double(0x7ff8000000000000ll);
                f[u] = in && flip[g] != 0;
            }
#pragma unroll
            for (uint32_t u = 0; u < PROF_UNROLL; ++u) {
                bool called, outside;
                const unsigned long long key = prof_key(x[u], f[u], called, outside);
                any_outside = any_outside || outside;
                if (!called) continue;
                const uint32_t digit = (uint32_t)(key >> shift) & (PROF_BINS - 1);
                const unsigned long long above = key >> shift >> 8;
                if (pass == 0) {
                    const double v = __longlong_as_double((long long)key);
                    ++n_called; n_gt0 += v > 0.0; n_ge5 += v >= 5.0; n_eq0 += v == 0.0; n_eq100 += v == 100.0;
                }
                if (above == want0) atomicAdd(&hist[0][digit * PROF_COLS + col], 1u);
                if (two && above == want1) atomicAdd(&hist[1][digit * PROF_COLS + col], 1u);
            }
        }
        if (pass == 0) {
            if (n_called) {
                atomicAdd(&cnt[0][col], n_called); atomicAdd(&cnt[1][col], n_gt0); atomicAdd(&cnt[2][col], n_ge5);
                atomicAdd(&cnt[3][col], n_eq0); atomicAdd(&cnt[4][col], n_eq100);
            }
            if (any_outside) atomicOr(bad_flag, 1u);
        }
        __syncthreads();
        if (tid < PROF_COLS && cnt[0][tid] != 0) {                     // one lane per column walks its 256 bins
            const uint32_t n = cnt[0][tid];
            const bool was_two = split[tid] != 0;
            const uint32_t r0 = pass ? rank[0][tid] : (n - 1) / 2, r1 = pass ? rank[1][tid] : n / 2;
            uint32_t cum0 = 0, cum1 = 0, b0 = PROF_BINS, b1 = PROF_BINS, in0 = 0, in1 = 0;
            for (uint32_t b = 0; b < PROF_BINS; ++b) {
                const uint32_t h0 = hist[0][b * PROF_COLS + tid], h1 = was_two ? hist[1][b * PROF_COLS + tid] : h0;
                if (b0 == PROF_BINS && r0 - cum0 < h0) { b0 = b; in0 = r0 - cum0; }
                if (b1 == PROF_BINS && r1 - cum1 < h1) { b1 = b; in1 = r1 - cum1; }
                if (b0 == PROF_BINS) cum0 += h0;
                if (b1 == PROF_BINS) cum1 += h1;
            }
            b0 &= PROF_BINS - 1; b1 &= PROF_BINS - 1;                  // a rank is always inside its prefix's count; never an index out of range
            const unsigned long long p0 = pfx[0][tid], p1 = was_two ? pfx[1][tid] : p0;
            pfx[0][tid] = p0 | (unsigned long long)b0 << shift;
            pfx[1][tid] = p1 | (unsigned long long)b1 << shift;
            rank[0][tid] = in0; rank[1][tid] = in1;
            if (!was_two && b0 != b1) split[tid] = 1;
        }
        __syncthreads();
    }
    if (tid < PROF_COLS && blockIdx.x * PROF_COLS + tid < n_cols) {
        const uint32_t cc = blockIdx.x * PROF_COLS + tid, n = cnt[0][tid];
        for (uint32_t i = 0; i < 5; ++i) counts[(size_t)i * ld + cc] = cnt[i][tid];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        mids[cc] = n ? __longlong_as_double((long long)pfx[0][tid]) : nan;
        mids[(size_t)ld + cc] = n ? __longlong_as_double((long long)pfx[1][tid]) : nan;
    }
}

int dev_profile_columns(const double *rows, uint32_t n_rows, uint32_t S, const uint8_t *flip, uint32_t cols_per_pass, void *stream_, uint32_t *counts[5],
                        double *mid_lo, double *mid_hi, bool *outside, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    *outside = false;
    // bands of columns that fit the device: a column's cells and 36 bytes of results
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const uint64_t per_col = (uint64_t)n_rows * 8 + 36;
    uint64_t band = cols_per_pass ? cols_per_pass : (uint64_t)(free_b * 0.5) / per_col;
    band = std::min<uint64_t>(band, S);
    if (band == 0) return fail(MSNV_ENOMEM, "subspecies profile: %llu bytes of device memory left, one column takes %llu", (unsigned long long)free_b, (unsigned long long)per_col);
    if (!cols_per_pass && band < S && band > PROF_COLS) band -= band % PROF_COLS;       // whole workgroups, rows that start on a 128-byte line
    const uint32_t ld = (uint32_t)band;
    Buf d_rows, d_flip, d_counts, d_mids, d_flag;
    MSNV_TRY(d_rows.alloc((size_t)n_rows * ld * 8));
    MSNV_TRY(d_flip.upload(flip, n_rows, st));
    MSNV_TRY(d_counts.alloc((size_t)5 * ld * 4));
    MSNV_TRY(d_mids.alloc((size_t)2 * ld * 8));
    MSNV_TRY(d_flag.alloc(4));
    HIP_TRY(hipMemsetAsync(d_flag.p, 0, 4, st));
    KernelTimer tm;
    std::vector<uint32_t> h_counts((size_t)5 * ld);
    std::vector<double> h_mids((size_t)2 * ld);
    for (uint32_t c0 = 0; c0 < S; c0 += ld) {
        const uint32_t nc = std::min(ld, S - c0);
        if (nc == S) HIP_TRY(hipMemcpyAsync(d_rows.p, rows, (size_t)n_rows * S * 8, hipMemcpyHostToDevice, st));
        else HIP_TRY(hipMemcpy2DAsync(d_rows.p, (size_t)ld * 8, rows + c0, (size_t)S * 8, (size_t)nc * 8, n_rows, hipMemcpyHostToDevice, st));
        MSNV_TRY(tm.begin(st));
        hipLaunchKernelGGL(msnv_profile_columns_k, dim3((nc + PROF_COLS - 1) / PROF_COLS), dim3(PROF_WAVES * 64), 0, st, d_rows.as<double>(), n_rows, ld, nc,
                           d_flip.as<uint8_t>(), d_counts.as<uint32_t>(), d_mids.as<double>(), d_flag.as<uint32_t>());
        MSNV_TRY(tm.stop(st));
        HIP_TRY(hipMemcpyAsync(h_counts.data(), d_counts.p, h_counts.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_mids.data(), d_mids.p, h_mids.size() * 8, hipMemcpyDeviceToHost, st));
        MSNV_TRY(tm.wait(st));
        for (uint32_t i = 0; i < 5; ++i) std::copy_n(h_counts.data() + (size_t)i * ld, nc, counts[i] + c0);
        std::copy_n(h_mids.data(), nc, mid_lo + c0);
        std::copy_n(h_mids.data() + ld, nc, mid_hi + c0);
    }
    uint32_t flag = 0;
    HIP_TRY(hipMemcpy(&flag, d_flag.p, 4, hipMemcpyDeviceToHost));
    *outside = flag != 0;
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
