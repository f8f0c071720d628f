// metasnv_amd/csrc/genecorr_k.hip -- subpopr's correlateSubpopProfileWithGeneProfiles (src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R)
// on the device: every cluster's abundance vector against every gene family's, Spearman and Pearson, with cor.test's derived columns
// and p.adjust(method = "BH").  Everything is fp64.
//
//   msnv_gc_min_positive   :123-124   min(x[x > 0]) of the kept gene matrix (the host divides by 1000: the pseudocount)
//   msnv_gc_cluster_rows   :141-153   ranks and log10(v + pseudocount) of the K + 1 cluster vectors, centred, into a global table
//   msnv_gc_gene_rows      :141-153   one workgroup per gene row: rank it in LDS, correlate it with every cluster vector
//   msnv_gc_stats          cor.test   statistic, two-sided p from the t distribution, Fisher interval: one thread per table row
//   msnv_bh_*              p.adjust   sort p descending, running minimum of (N / rank) * p capped at 1, scattered back
//
// Ranking one row of S samples (rank_row): P = the next power of two (>= 64), T = min(P, 1024) threads.
//   LDS, carved from the dynamic block:   key[P] f64 | idx[P] u16 | first[P] u16 | last[P] u16   = 14 P bytes (112 KiB at the cap, P = 8192)
//   1. the row, coalesced, into key[] (padding +inf), idx[i] = i
//   2. bitonic sort of (key, idx)
//   3. tie runs: first[i] = max-scan forwards of "i where a run starts", last[i] = min-scan backwards of "i where a run ends";
//      twice the average rank of position i is first + last + 2 (<= 2 P: 16 bits)
//   4. every thread takes its positions' rank, log10(key + pc) and idx into registers, then scatters them to sample order:
//      first[] becomes the ranks by sample, key[] the logs by sample (in place: all reads precede the barrier)
// The sums are reduced in one fixed order (strided per thread, a butterfly inside a wavefront, the wavefronts in turn), which
// depends on S alone; a gene row and a cluster row are ranked and centred by the same code, so equal vectors give equal bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

namespace msnv {

namespace {

constexpr uint32_t GC_THREADS = 1024, GC_PER_THREAD = GENECORR_MAX_SAMPLES / GC_THREADS;
static_assert(GENECORR_MAX_SAMPLES <= 32768 && (GENECORR_MAX_SAMPLES & (GENECORR_MAX_SAMPLES - 1)) == 0, "twice a rank must fit 16 bits");

struct RowLds { double *key; uint16_t *idx, *first, *last; };

__device__ inline RowLds carve(unsigned char *base, uint32_t P) {
    RowLds L;
    L.key = (double *)base;
    L.idx = (uint16_t *)(base + (size_t)P * 8);
    L.first = L.idx + P;
    L.last = L.first + P;
    return L;
}

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Sum of a and of b over the workgroup, the same value in every thread.  red: 2 * 16 doubles of static LDS.
__device__ inline void block_sum2(double &a, double &b, double *red) {
    a = wave_sum(a); b = wave_sum(b);
    const uint32_t w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[16 + w] = b; }
    __syncthreads();
    a = red[0]; b = red[16];
    for (uint32_t i = 1; i < nw; ++i) { a += red[i]; b += red[16 + i]; }
    __syncthreads();
}

// Leaves L.first[s] = twice the average rank of sample s and L.key[s] = log10(row[s] + pc); returns max != min.
// *bad is set when a cell is negative, NaN or infinite (the result of that row is then meaningless, the indices stay in range).
__device__ bool rank_row(const double *__restrict__ row, uint32_t S, uint32_t P, double pc, const RowLds &L, uint32_t *bad) {
    const uint32_t T = blockDim.x, tid = threadIdx.x;
    for (uint32_t i = tid; i < P; i += T) {
        double v = __longlong_as_double(0x7ff0000000000000ll);
        if (i < S) {
            v = row[i];
            if (!(v >= 0.0 && v < __longlong_as_double(0x7ff0000000000000ll))) *bad = 1;
        }
        L.key[i] = v;
        L.idx[i] = (uint16_t)i;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += T) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                const double a = L.key[i], b = L.key[q];
                const uint16_t ia = L.idx[i], ib = L.idx[q];
                const bool gt = a > b || (a == b && ia > ib);
                if (gt == ((i & k) == 0)) { L.key[i] = b; L.key[q] = a; L.idx[i] = ib; L.idx[q] = ia; }
            }
            __syncthreads();
        }
    const bool varies = L.key[0] != L.key[S - 1];
    for (uint32_t i = tid; i < P; i += T) {
        L.first[i] = (i == 0 || L.key[i] != L.key[i - 1]) ? (uint16_t)i : (uint16_t)0;
        L.last[i] = (i == P - 1 || L.key[i] != L.key[i + 1]) ? (uint16_t)i : (uint16_t)(P - 1);
    }
    __syncthreads();
    for (uint32_t d = 1; d < P; d <<= 1) {
        uint16_t f[GC_PER_THREAD], l[GC_PER_THREAD];
#pragma unroll
        for (uint32_t e = 0; e < GC_PER_THREAD; ++e) {
            const uint32_t i = tid + e * T;
            if (i < P) {
                f[e] = L.first[i]; l[e] = L.last[i];
                if (i >= d) f[e] = max(f[e], L.first[i - d]);
                if (i + d < P) l[e] = min(l[e], L.last[i + d]);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < GC_PER_THREAD; ++e) {
            const uint32_t i = tid + e * T;
            if (i < P) { L.first[i] = f[e]; L.last[i] = l[e]; }
        }
        __syncthreads();
    }
    uint16_t r2[GC_PER_THREAD], id[GC_PER_THREAD];
    double lg[GC_PER_THREAD];
#pragma unroll
    for (uint32_t e = 0; e < GC_PER_THREAD; ++e) {
        const uint32_t i = tid + e * T;
        if (i < S) { r2[e] = (uint16_t)(L.first[i] + L.last[i] + 2u); id[e] = L.idx[i]; lg[e] = log10(L.key[i] + pc); }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t e = 0; e < GC_PER_THREAD; ++e) {
        const uint32_t i = tid + e * T;
        if (i < S) { const uint32_t s = id[e] < S ? id[e] : 0u; L.first[s] = r2[e]; L.key[s] = lg[e]; }
    }
    __syncthreads();
    return varies;
}

// mean of the logs, then the centred sums of squares of ranks and logs (two-pass; the rank mean is exactly (S + 1) / 2)
__device__ inline void row_moments(const RowLds &L, uint32_t S, double *red, double &mean_log, double &ss_rank, double &ss_log) {
    const uint32_t T = blockDim.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (uint32_t s = tid; s < S; s += T) a += L.key[s];
    block_sum2(a, b, red);
    mean_log = a / (double)S;
    const double mr = 0.5 * (double)(S + 1);
    a = 0.0; b = 0.0;
    for (uint32_t s = tid; s < S; s += T) {
        const double dr = 0.5 * (double)L.first[s] - mr, dl = L.key[s] - mean_log;
        a += dr * dr; b += dl * dl;
    }
    block_sum2(a, b, red);
    ss_rank = a; ss_log = b;
}

__device__ inline double corr_of(double sxy, double sxx, double syy) {
    const double c = sxy / sqrt(sxx * syy);
    return c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
}

}  // namespace

extern __shared__ __align__(16) unsigned char gc_lds[];

// bits of the smallest positive cell (positive doubles order like their bit patterns); *out starts at all ones
__global__ void msnv_gc_min_positive(const double *x, uint64_t n, unsigned long long *out) {
    unsigned long long m = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double v = x[i];
        if (v > 0.0) m = min(m, (unsigned long long)__double_as_longlong(v));
    }
    for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned long long)__shfl_xor((long long)m, o));
    if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(out, m);
}

// cluster c: centred ranks and logs by sample into crank / clog [K1][S], csum[c] = {sum of squares of ranks, of logs}, cvalid[c]
__global__ void __launch_bounds__(GC_THREADS) msnv_gc_cluster_rows(const double *clust, uint32_t S, uint32_t P, double pc, double *crank, double *clog,
                                                                   double *csum, uint8_t *cvalid, uint32_t *bad) {
    __shared__ double red[32];
    const RowLds L = carve(gc_lds, P);
    const uint32_t c = blockIdx.x;
    const bool varies = rank_row(clust + (uint64_t)c * S, S, P, pc, L, bad);
    double ml, ssr, ssl;
    row_moments(L, S, red, ml, ssr, ssl);
    const double mr = 0.5 * (double)(S + 1);
    for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) {
        crank[(uint64_t)c * S + s] = 0.5 * (double)L.first[s] - mr;
        clog[(uint64_t)c * S + s] = L.key[s] - ml;
    }
    if (threadIdx.x == 0) { csum[2 * c] = ssr; csum[2 * c + 1] = ssl; cvalid[c] = varies ? 1 : 0; }
}

// gene row g0 + blockIdx.x of the chunk `genes` ([rows][S]): rho / r / valid at [c * G + g]
__global__ void __launch_bounds__(GC_THREADS) msnv_gc_gene_rows(const double *genes, uint32_t S, uint32_t P, double pc, uint32_t K1, const double *crank,
                                                                const double *clog, const double *csum, const uint8_t *cvalid, uint64_t G, uint64_t g0,
                                                                double *rho, double *r, uint8_t *valid, uint32_t *bad) {
    __shared__ double red[32];
    const RowLds L = carve(gc_lds, P);
    const uint64_t g = g0 + blockIdx.x;
    const bool varies = rank_row(genes + (uint64_t)blockIdx.x * S, S, P, pc, L, bad);
    double ml, ssr, ssl;
    row_moments(L, S, red, ml, ssr, ssl);
    const double mr = 0.5 * (double)(S + 1);
    for (uint32_t c = 0; c < K1; ++c) {
        double a = 0.0, b = 0.0;
        const double *cr = crank + (uint64_t)c * S, *cl = clog + (uint64_t)c * S;
        for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) {
            const double dr = 0.5 * (double)L.first[s] - mr, dl = L.key[s] - ml;
            a += cr[s] * dr; b += cl[s] * dl;
        }
        block_sum2(a, b, red);
        if (threadIdx.x == 0) {
            const bool ok = varies && cvalid[c];
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            rho[(uint64_t)c * G + g] = ok ? corr_of(a, csum[2 * c], ssr) : nan;
            r[(uint64_t)c * G + g] = ok ? corr_of(b, csum[2 * c + 1], ssl) : nan;
            valid[(uint64_t)c * G + g] = ok ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------- cor.test's derived columns
namespace {

// continued fraction of the incomplete beta function, modified Lentz
__device__ double beta_cf(double a, double b, double x) {
    const double tiny = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 20000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 3e-16) break;
    }
    return h;
}

// Gamma(a + 1/2) / Gamma(a) to an ulp or two: shifted up to a >= 20 by the recurrence, then the asymptotic series.  (The difference of two
// lgamma values of size 250, at df = 148, leaves 1e-13 of relative error in the density and ten times that in a p of 0.09 taken as 1 - I.)
__device__ double gamma_ratio(double a) {
    double pr = 1.0, z = a;
    while (z < 20.0) { pr *= z / (z + 0.5); z += 1.0; }
    const double w = 1.0 / z, w2 = w * w;
    return pr * sqrt(z) * exp(w * (-1.0 / 8.0 + w2 * (1.0 / 192.0 + w2 * (-1.0 / 640.0 + w2 * (17.0 / 14336.0 + w2 * (-31.0 / 18432.0))))));
}

// cor.test's t with R's own rounding: sqrt(df) e / sqrt(1 - e^2) for pearson, e / sqrt((1 - e^2) / df) for spearman.  Contraction is off:
// fused into one fma, 1 - e * e is closer to the truth and further from what R prints (5e-12 of the statistic at e = 0.999999).
__device__ double t_statistic(int method, double e, double df) {
#pragma clang fp contract(off)
    const double ee = e * e, u = 1.0 - ee;
    if (u <= 0.0) return e > 0 ? __longlong_as_double(0x7ff0000000000000ll) : __longlong_as_double(0xfff0000000000000ll);
    if (method == 0) { const double num = sqrt(df) * e; return num / sqrt(u); }
    const double v = u / df;
    return e / sqrt(v);
}

// spearman's S = (n^3 - n)(1 - e) / 6, every operation rounded on its own
__device__ double spearman_s(double e, double n) {
#pragma clang fp contract(off)
    const double n3 = n * n * n, a = n3 - n, b = 1.0 - e, ab = a * b;
    return ab / 6.0;
}

// min(1, 2 P(T_df >= |t|)) = I_x(df / 2, 1 / 2) at x = df / (df + t^2)
__device__ double t_two_sided(double t, double df) {
    if (isinf(t)) return 0.0;
    if (t == 0.0) return 1.0;
    const double t2 = t * t, x = df / (df + t2), y = t2 / (df + t2), a = 0.5 * df, b = 0.5;
    const double lx = y < 0.5 ? log1p(-y) : log(x);
    const double front = exp(a * lx) * sqrt(y) * gamma_ratio(a) / 1.7724538509055159;      // x^a y^b / B(a, b)
    const double p = x < (a + 1.0) / (a + b + 2.0) ? front * beta_cf(a, b, x) / a : 1.0 - front * beta_cf(b, a, y) / b;
    return p > 1.0 ? 1.0 : (p < 0.0 ? 0.0 : p);
}

}  // namespace

// method 0 pearson: statistic = t, interval tanh(atanh(e) -+ qnorm(0.975) / sqrt(n - 3)) (NaN at n = 3);
// method 1 spearman: statistic = (n^3 - n)(1 - e) / 6
__global__ void msnv_gc_stats(int method, uint64_t n_rows, const double *est, const int32_t *n_obs, double *stat, double *p, double *lo, double *hi) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const double e = est[i], n = (double)n_obs[i], df = n - 2.0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double t = t_statistic(method, e, df);
    if (method == 0) {
        stat[i] = t;
        if (lo && hi) {
            if (n_obs[i] > 3) {
                const double z = atanh(e), s = 1.959963984540054 / sqrt(n - 3.0);
                lo[i] = tanh(z - s); hi[i] = tanh(z + s);
            } else { lo[i] = nan; hi[i] = nan; }
        }
    } else {
        stat[i] = spearman_s(e, n);
    }
    p[i] = t_two_sided(t, df);
}

// ---------------------------------------------------------------------------------------------- Benjamini-Hochberg
namespace {
constexpr uint32_t BH_TILE = 2048, BH_THREADS = 1024;
// the order of the sort: p descending, then index ascending (a total order: the result does not depend on the launch)
__device__ inline bool bh_before(double pa, uint32_t ia, double pb, uint32_t ib) { return pa > pb || (pa == pb && ia < ib); }
}  // namespace

__global__ void msnv_bh_init(const double *p, uint64_t n, uint64_t n_pad, double *key, uint32_t *idx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    key[i] = i < n ? p[i] : __longlong_as_double(0xfff0000000000000ll);      // padding sorts last
    idx[i] = (uint32_t)i;
}

// every step with a distance below the tile, in LDS: for k = k_first .. k_last, j = min(k / 2, tile / 2) .. 1
__global__ void __launch_bounds__(BH_THREADS) msnv_bh_sort_tile(double *key, uint32_t *idx, uint32_t tile, uint64_t k_first, uint64_t k_last) {
    __shared__ double sk[BH_TILE];
    __shared__ uint32_t si[BH_TILE];
    const uint64_t base = (uint64_t)blockIdx.x * tile;
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) { sk[i] = key[base + i]; si[i] = idx[base + i]; }
    __syncthreads();
    for (uint64_t k = k_first; k <= k_last; k <<= 1)
        for (uint32_t j = (uint32_t)min(k >> 1, (uint64_t)(tile >> 1)); j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < tile / 2; t += blockDim.x) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                const double a = sk[i], b = sk[q];
                const uint32_t ia = si[i], ib = si[q];
                const bool up = ((base + i) & k) == 0;
                if (bh_before(b, ib, a, ia) == up) { sk[i] = b; sk[q] = a; si[i] = ib; si[q] = ia; }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) { key[base + i] = sk[i]; idx[base + i] = si[i]; }
}

// one step with a distance of a tile or more, in global memory: one thread per pair
__global__ void msnv_bh_sort_step(double *key, uint32_t *idx, uint64_t n_pad, uint64_t k, uint64_t j) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pad / 2) return;
    const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
    const double a = key[i], b = key[q];
    const uint32_t ia = idx[i], ib = idx[q];
    if (bh_before(b, ib, a, ia) == ((i & k) == 0)) { key[i] = b; key[q] = a; idx[i] = ib; idx[q] = ia; }
}

// one workgroup: position i of the descending order has rank n - i; q = min(1, running minimum of (n / rank) * p), scattered to idx
__global__ void __launch_bounds__(BH_THREADS) msnv_bh_scan(const double *key, const uint32_t *idx, uint64_t n, double *q) {
    __shared__ double sm[BH_THREADS];
    const uint64_t chunk = (n + BH_THREADS - 1) / BH_THREADS;
    const uint64_t lo = min(n, (uint64_t)threadIdx.x * chunk), hi = min(n, lo + chunk);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double m = inf;
    for (uint64_t i = lo; i < hi; ++i) m = fmin(m, ((double)n / (double)(n - i)) * key[i]);
    sm[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t d = 1; d < BH_THREADS; d <<= 1) {
        const double o = threadIdx.x >= d ? sm[threadIdx.x - d] : inf;
        __syncthreads();
        sm[threadIdx.x] = fmin(sm[threadIdx.x], o);
        __syncthreads();
    }
    m = threadIdx.x ? sm[threadIdx.x - 1] : inf;
    for (uint64_t i = lo; i < hi; ++i) {
        m = fmin(m, ((double)n / (double)(n - i)) * key[i]);
        q[idx[i]] = fmin(1.0, m);
    }
}

// ---------------------------------------------------------------------------------------------- host side of the launches
namespace {

inline uint32_t pad_pow2(uint32_t s) { uint32_t p = 64; while (p < s) p <<= 1; return p; }

}  // namespace

int dev_gene_corr(uint32_t K1, uint64_t G, uint32_t S, const double *clust, const double *genes, void *stream_, double *rho, double *r,
                  uint8_t *valid, double *pseudocount, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    const uint32_t P = pad_pow2(S), T = std::min(P, GC_THREADS);
    const size_t lds = (size_t)P * 14;
    if (lds > 48 * 1024) {
        HIP_TRY(hipFuncSetAttribute((const void *)msnv_gc_cluster_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(hipFuncSetAttribute((const void *)msnv_gc_gene_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    const uint64_t row_bytes = (uint64_t)S * 8, n_out = (uint64_t)K1 * G;
    Buf d_clust, d_crank, d_clog, d_csum, d_cvalid, d_flags, d_rho, d_r, d_valid, d_genes;
    MSNV_TRY(d_clust.upload(clust, K1 * row_bytes, st));
    MSNV_TRY(d_crank.alloc(K1 * row_bytes));
    MSNV_TRY(d_clog.alloc(K1 * row_bytes));
    MSNV_TRY(d_csum.alloc((size_t)K1 * 16));
    MSNV_TRY(d_cvalid.alloc(K1));
    MSNV_TRY(d_flags.alloc(16));                                       // [0..7] bits of the smallest positive cell, [8..11] bad-cell flag
    MSNV_TRY(d_rho.alloc(n_out * 8));
    MSNV_TRY(d_r.alloc(n_out * 8));
    MSNV_TRY(d_valid.alloc(n_out));
    // the gene matrix in row chunks that fit the device: whole when it does (then it is uploaded once for both passes)
    uint64_t chunk_rows = 0;
    MSNV_TRY(slab_rows(G, row_bytes, 0.8, 0x7fffffffull, "gene correlation", &chunk_rows));
    MSNV_TRY(d_genes.alloc(chunk_rows * row_bytes));
    const bool whole = chunk_rows >= G;
    KernelTimer tm;
    HIP_TRY(hipMemsetAsync(d_flags.p, 0xff, 8, st));
    HIP_TRY(hipMemsetAsync((char *)d_flags.p + 8, 0, 8, st));
    // pass 1: the pseudocount, finished before anything takes a logarithm
    for (uint64_t g0 = 0; g0 < G; g0 += chunk_rows) {
        const uint64_t rows = std::min(chunk_rows, G - g0), cells = rows * S;
        HIP_TRY(hipMemcpyAsync(d_genes.p, genes + g0 * S, rows * row_bytes, hipMemcpyHostToDevice, st));
        MSNV_TRY(tm.begin(st));
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((cells + 255) / 256, dev_resident_workgroups(8));
        hipLaunchKernelGGL(msnv_gc_min_positive, dim3(blocks), dim3(256), 0, st, d_genes.as<double>(), cells, d_flags.as<unsigned long long>());
        MSNV_TRY(tm.end(st));
    }
    unsigned long long min_bits = 0;
    HIP_TRY(hipMemcpy(&min_bits, d_flags.p, 8, hipMemcpyDeviceToHost));
    if (min_bits == ~0ull) return fail(MSNV_EDOMAIN, "gene correlation: the gene matrix holds no cell above 0 (the reference's pseudocount is the smallest such cell / 1000)");
    double min_pos;
    memcpy(&min_pos, &min_bits, 8);
    const double pc = min_pos / 1000.0;
    uint32_t *bad = (uint32_t *)((char *)d_flags.p + 8);
    MSNV_TRY(tm.begin(st));
    hipLaunchKernelGGL(msnv_gc_cluster_rows, dim3(K1), dim3(T), lds, st, d_clust.as<double>(), S, P, pc, d_crank.as<double>(), d_clog.as<double>(),
                       d_csum.as<double>(), d_cvalid.as<uint8_t>(), bad);
    MSNV_TRY(tm.end(st));
    // pass 2: one workgroup per gene row
    for (uint64_t g0 = 0; g0 < G; g0 += chunk_rows) {
        const uint64_t rows = std::min(chunk_rows, G - g0);
        if (!whole) HIP_TRY(hipMemcpyAsync(d_genes.p, genes + g0 * S, rows * row_bytes, hipMemcpyHostToDevice, st));
        MSNV_TRY(tm.begin(st));
        hipLaunchKernelGGL(msnv_gc_gene_rows, dim3((uint32_t)rows), dim3(T), lds, st, d_genes.as<double>(), S, P, pc, K1, d_crank.as<double>(), d_clog.as<double>(),
                           d_csum.as<double>(), d_cvalid.as<uint8_t>(), G, g0, d_rho.as<double>(), d_r.as<double>(), d_valid.as<uint8_t>(), bad);
        MSNV_TRY(tm.end(st));
    }
    uint32_t bad_host = 0;
    HIP_TRY(hipMemcpy(&bad_host, bad, 4, hipMemcpyDeviceToHost));
    if (bad_host) return fail(MSNV_EDOMAIN, "gene correlation: a negative, NaN or infinite abundance (abundances are >= 0 and finite)");
    HIP_TRY(hipMemcpy(rho, d_rho.p, n_out * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r, d_r.p, n_out * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, d_valid.p, n_out, hipMemcpyDeviceToHost));
    if (pseudocount) *pseudocount = pc;
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

int dev_corr_stats(int method, uint64_t n, const double *est, const int32_t *n_obs, void *stream_, double *stat, double *p, double *lo, double *hi, double *q) {
    hipStream_t st = (hipStream_t)stream_;
    if (!n) return MSNV_OK;
    uint64_t n_pad = 2;
    while (n_pad < n) n_pad <<= 1;
    const bool ci = method == 0 && lo && hi;
    Buf d_est, d_nobs, d_stat, d_p, d_lo, d_hi, d_q, d_key, d_idx;
    MSNV_TRY(d_est.upload(est, n * 8, st)); MSNV_TRY(d_nobs.upload(n_obs, n * 4, st));
    MSNV_TRY(d_stat.alloc(n * 8)); MSNV_TRY(d_p.alloc(n * 8)); MSNV_TRY(d_q.alloc(n * 8));
    if (ci) { MSNV_TRY(d_lo.alloc(n * 8)); MSNV_TRY(d_hi.alloc(n * 8)); }
    MSNV_TRY(d_key.alloc(n_pad * 8)); MSNV_TRY(d_idx.alloc(n_pad * 4));
    hipLaunchKernelGGL(msnv_gc_stats, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, method, n, d_est.as<double>(), d_nobs.as<int32_t>(), d_stat.as<double>(),
                       d_p.as<double>(), d_lo.as<double>(), d_hi.as<double>());
    hipLaunchKernelGGL(msnv_bh_init, dim3((uint32_t)((n_pad + 255) / 256)), dim3(256), 0, st, d_p.as<double>(), n, n_pad, d_key.as<double>(), d_idx.as<uint32_t>());
    const uint32_t tile = (uint32_t)std::min<uint64_t>(n_pad, BH_TILE), n_tiles = (uint32_t)(n_pad / tile);
    hipLaunchKernelGGL(msnv_bh_sort_tile, dim3(n_tiles), dim3(BH_THREADS), 0, st, d_key.as<double>(), d_idx.as<uint32_t>(), tile, (uint64_t)2, (uint64_t)tile);
    for (uint64_t k = (uint64_t)tile << 1; k <= n_pad; k <<= 1) {           // merging tiles
        for (uint64_t j = k >> 1; j >= tile; j >>= 1)
            hipLaunchKernelGGL(msnv_bh_sort_step, dim3((uint32_t)((n_pad / 2 + 255) / 256)), dim3(256), 0, st, d_key.as<double>(), d_idx.as<uint32_t>(), n_pad, k, j);
        hipLaunchKernelGGL(msnv_bh_sort_tile, dim3(n_tiles), dim3(BH_THREADS), 0, st, d_key.as<double>(), d_idx.as<uint32_t>(), tile, k, k);
    }
    hipLaunchKernelGGL(msnv_bh_scan, dim3(1), dim3(BH_THREADS), 0, st, d_key.as<double>(), d_idx.as<uint32_t>(), n, d_q.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(stat, d_stat.p, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(p, d_p.p, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(q, d_q.p, n * 8, hipMemcpyDeviceToHost, st));
    if (ci) {
        HIP_TRY(hipMemcpyAsync(lo, d_lo.p, n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hi, d_hi.p, n * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MSNV_OK;
}

}  // namespace msnv
