// metasnv_amd/csrc/genotype_k.hip -- subpopr's computeUniquePosPerCluster on the device (src/subpopr/R/writeGenotypeFreqs.R:195-277; the
// host side is genotype.cpp, the rule is stated in include/msnv.h).
//
//   msnv_genotype_rows_k   per row of the SNV frequency table: which clusters it genotypes (select), which of those have the minor allele
//                          as their majority (flip), and whether one of its mean differences lies within GENO_GUARD of the threshold (near, bit 0
//                          of its flag byte; bit 1: a cell outside [0, 100])
//
// One wavefront per table row, grid-strided: a row is contiguous, so the lanes read it coalesced through the column list (col[] in cluster
// order, seg[k] the first entry of cluster k; columns not in use are not listed).  Per cluster every lane sums its share of the segment --
// the fp64 sum of the non-NaN cells, the NaN count, the count of cells < 50 -- and a butterfly of shuffles leaves the totals in every lane;
// lane k keeps cluster k's (a lane-indexed register: no array, no LDS, no scratch).  Lane i < K then reads every other cluster's mean with a
// shuffle and evaluates the three conditions; ballots form the masks and lane 0 stores them.  The NaN proportions are integer counts
// and one IEEE division, exact; the means are fp64 sums in butterfly order, and a comparison that GENO_GUARD cannot decide is redone on
// the host in long double (genotype.cpp), so the masks are the long double rule's on every row.
// The grid is GENO_GRID_BLOCKS workgroups of GENO_ROWS_PER_BLOCK wavefronts at the most (256 CUs x 8): a table with more rows than that
// takes further trips.  The table goes up in slabs of GENO_SLAB_BYTES at the most, less when the device has less to give.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

#pragma clang fp contract(off)

namespace msnv {

__global__ void __launch_bounds__(GENO_ROWS_PER_BLOCK * 64) msnv_genotype_rows_k(const double *__restrict__ rows, unsigned long long n_rows, uint32_t S,
                                                                                 const uint32_t *__restrict__ col, const uint32_t *__restrict__ seg, uint32_t K,
                                                                                 double threshold, uint32_t *__restrict__ select_mask, uint32_t *__restrict__ flip_mask,
                                                                                 uint8_t *__restrict__ near_flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * GENO_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const unsigned long long n_waves = (unsigned long long)gridDim.x * GENO_ROWS_PER_BLOCK;
    const uint32_t n_used = seg[K];
    const uint32_t my_lo = lane < K ? seg[lane] : 0u, my_size = lane < K ? seg[lane + 1] - my_lo : 0u;
    for (unsigned long long p = wave; p < n_rows; p += n_waves) {
        const double *__restrict__ row = rows + (size_t)p * S;
        double my_sum = 0.0;
        uint32_t my_na = 0, my_lt = 0, all_na = 0;
        bool outside = false;                                          // a cell that is neither NaN nor within [0, 100]: the host refuses the table
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t lo = seg[k], hi = seg[k + 1];
            double sum = 0.0;
            uint32_t na = 0, lt = 0;
            for (uint32_t c = lo + lane; c < hi; c += 64) {
                const double x = row[col[c]];
                if (x != x) ++na;
                else { sum += x; lt += x < 50.0 ? 1u : 0u; outside = outside || !(x >= 0.0 && x <= 100.0); }
            }
            for (int o = 32; o > 0; o >>= 1) {
                sum += __shfl_xor(sum, o);
                na += (uint32_t)__shfl_xor((int)na, o);
                lt += (uint32_t)__shfl_xor((int)lt, o);
            }
            all_na += na;
            if (lane == k) { my_sum = sum; my_na = na; my_lt = lt; }
        }
        // lane i < K: cluster i
        const uint32_t valid = my_size - my_na;
        const double mean = my_sum / (double)valid;                    // 0 / 0 = NaN: a cluster without a cell on this row
        const bool na_in = (double)my_na / (double)my_size < 0.2;
        const bool na_out = (double)(all_na - my_na) / (double)(n_used - my_size) < 0.2;
        bool distinct = true, near = false;
        for (uint32_t j = 0; j < K; ++j) {
            const double mj = __shfl(mean, (int)j);
            if (j == lane) continue;
            double f = fabs(mean - mj);
            if (f != f) f = 0.0;                                       // fDist[is.na(fDist)] <- 0
            distinct = distinct && f > threshold;
            near = near || fabs(f - threshold) <= GENO_GUARD;
        }
        const bool sel = lane < K && na_in && na_out && distinct;
        const bool flip = sel && my_lt > valid - my_lt;                // median of the 0 / 1 vector is 0: zeros outnumber ones
        const unsigned long long sel_b = __ballot(sel), flip_b = __ballot(flip), near_b = __ballot(lane < K && near), out_b = __ballot(outside);
        if (lane == 0) {
            select_mask[p] = (uint32_t)sel_b;
            flip_mask[p] = (uint32_t)flip_b;
            near_flag[p] = (uint8_t)((near_b ? 1 : 0) | (out_b ? 2 : 0));
        }
    }
}

int dev_genotype_rows(const double *rows, uint64_t n_pos, uint32_t S, const uint32_t *col, const uint32_t *seg, uint32_t K, double threshold, void *stream_,
                      uint32_t *select_mask, uint32_t *flip_mask, uint8_t *near_flag, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    if (n_pos == 0) return MSNV_OK;
    const uint32_t n_used = seg[K];
    Buf d_rows, d_col, d_seg, d_sel, d_flip, d_near;
    MSNV_TRY(d_col.upload(col, (size_t)n_used * 4, st));
    MSNV_TRY(d_seg.upload(seg, (size_t)(K + 1) * 4, st));
    // row slabs that fit the device: the table's slab and 9 bytes of results per row
    const uint64_t row_bytes = (uint64_t)S * 8;
    uint64_t chunk = 0;
    MSNV_TRY(slab_rows(n_pos, row_bytes + 9, 0.5, std::max<uint64_t>(1, GENO_SLAB_BYTES / row_bytes), "genotyping positions", &chunk));
    MSNV_TRY(d_rows.alloc(chunk * row_bytes));
    MSNV_TRY(d_sel.alloc(chunk * 4));
    MSNV_TRY(d_flip.alloc(chunk * 4));
    MSNV_TRY(d_near.alloc(chunk));
    KernelTimer tm;
    for (uint64_t p0 = 0; p0 < n_pos; p0 += chunk) {
        const uint64_t np = std::min(chunk, n_pos - p0);
        HIP_TRY(hipMemcpyAsync(d_rows.p, rows + p0 * S, np * row_bytes, hipMemcpyHostToDevice, st));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((np + GENO_ROWS_PER_BLOCK - 1) / GENO_ROWS_PER_BLOCK, GENO_GRID_BLOCKS);
        MSNV_TRY(tm.begin(st));
        hipLaunchKernelGGL(msnv_genotype_rows_k, dim3(grid), dim3(GENO_ROWS_PER_BLOCK * 64), 0, st, d_rows.as<double>(), (unsigned long long)np, S, d_col.as<uint32_t>(),
                           d_seg.as<uint32_t>(), K, threshold, d_sel.as<uint32_t>(), d_flip.as<uint32_t>(), d_near.as<uint8_t>());
        MSNV_TRY(tm.stop(st));
        HIP_TRY(hipMemcpyAsync(select_mask + p0, d_sel.p, np * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(flip_mask + p0, d_flip.p, np * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(near_flag + p0, d_near.p, np, hipMemcpyDeviceToHost, st));
        MSNV_TRY(tm.wait(st));
    }
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
