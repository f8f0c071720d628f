// metasnv_amd/csrc/pcoa_k.hip -- subpopr's computePCoA on the device (src/subpopr/R/clustering.R:472-505, ape::pcoa(correction = "none"); the host
// side of the stage is pcoa.cpp).  The rule is in include/msnv.h; every arithmetic operation below is one fp64 operation, never contracted.
//
//   msnv_pcoa_rowmean_k   r_i = (sum over j ascending of -0.5 d_ij^2) / n: one lane per row, the sum inside the lane.  Lane i reads D[j * n + i] (the
//                         matrix is symmetric), so a wavefront reads one row per trip
//   msnv_pcoa_grand_k     g = (sum over i ascending of r_i) / n: one lane
//   msnv_pcoa_centre_k    B_ij = ((A_ij - r_i) - r_j) + g for i <= j, mirrored into j > i; V = I
//   msnv_pcoa_absmax_k    max |B_ij| as the largest bit pattern (non-negative doubles order like their bits): an integer atomic max, exact in any order
//   msnv_pcoa_diag_k      the diagonal, gathered for the host: the trace before the solve, the eigenvalues after it
//   msnv_pcoa_params_k    one lane per pair of step r: t, c, s and whether the pair rotates; adds the number of rotating pairs to a counter (integer atomic)
//   msnv_pcoa_rotate_k    one lane per 2 x 2 block I <= J of the matrix and per (row of V, pair): the block is read, transformed by the parameters of
//                         I and J and written to itself and, transposed, to its mirror.  Nobody reads the mirror, so the update is in place
//   msnv_pcoa_axes_k      one workgroup per axis: the first component of largest magnitude decides the sign, the column is scaled by sqrt(lambda)
//
// The pairs of step r come from r alone (pair_of): slot 0 is (m - 1, r), slot i is ((r + i) mod (m - 1), (r - i) mod (m - 1)), m = n + (n & 1).  For
// consecutive slots the first index ascends and the second descends by one, so the lanes of a wavefront (consecutive J) touch two runs of neighbouring
// columns of a row.  With n odd index n does not exist: slot 0 is then the bye, one row or column that takes only the other side's rotation.
// The steps of a sweep are queued behind each other on one stream, which is the only barrier between them; the host waits once per sweep for the
// 4-byte counter.  No sum of doubles crosses lanes anywhere, so the result is a function of the matrix alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

#pragma clang fp contract(off)

namespace msnv {

namespace {

constexpr uint32_t PAIR_THREADS = 128;                                 // msnv_pcoa_params_k: 513 samples are 257 slots, three workgroups
constexpr uint32_t ROT_X = 64, ROT_Y = 4;                              // msnv_pcoa_rotate_k: a wavefront along J
constexpr uint32_t AXIS_THREADS = 256;
constexpr unsigned long long NAN_BITS = 0x7ff8000000000000ull, INF_BITS = 0x7ff0000000000000ull;

struct Rot { double c, s, t; uint32_t rotates, pad; };                 // one pair's parameters; c = 1, s = t = 0 when it does not rotate

// slot i of step r: p < q, and q == n (an index that does not exist) for the bye of an odd n
__device__ __host__ inline void pair_of(uint32_t m, uint32_t r, uint32_t i, uint32_t &p, uint32_t &q) {
    const uint32_t m1 = m - 1;
    uint32_t a = m1, b = r;
    if (i) {
        a = r + i; if (a >= m1) a -= m1;
        b = r + m1 - i; if (b >= m1) b -= m1;
    }
    p = a < b ? a : b; q = a < b ? b : a;
}

}  // namespace

__global__ void __launch_bounds__(256) msnv_pcoa_rowmean_k(const double *__restrict__ D, uint32_t n, double *__restrict__ rmean) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (uint32_t j = 0; j < n; ++j) {
        const double d = D[(size_t)j * n + i];
        s += -0.5 * (d * d);
    }
    rmean[i] = s / (double)n;
}

__global__ void msnv_pcoa_grand_k(double *__restrict__ rmean, uint32_t n) {      // rmean[n] = g
    if (blockIdx.x || threadIdx.x) return;
    double s = 0.0;
    for (uint32_t i = 0; i < n; ++i) s += rmean[i];
    rmean[n] = s / (double)n;
}

__global__ void __launch_bounds__(256) msnv_pcoa_centre_k(const double *__restrict__ D, uint32_t n, const double *__restrict__ rmean, double *__restrict__ B,
                                                          double *__restrict__ V) {
    const uint32_t j = blockIdx.x * ROT_X + threadIdx.x, i = blockIdx.y * ROT_Y + threadIdx.y;
    if (j >= n || i > j) return;
    const double d = D[(size_t)i * n + j], a = -0.5 * (d * d);
    const double b = ((a - rmean[i]) - rmean[j]) + rmean[n];
    B[(size_t)i * n + j] = b; B[(size_t)j * n + i] = b;
    const double v = i == j ? 1.0 : 0.0;
    V[(size_t)i * n + j] = v; V[(size_t)j * n + i] = v;
}

__global__ void __launch_bounds__(256) msnv_pcoa_absmax_k(const double *__restrict__ B, unsigned long long cells, unsigned long long *__restrict__ max_bits) {
    __shared__ unsigned long long red[256];
    unsigned long long mx = 0;
    for (unsigned long long c = (unsigned long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (unsigned long long)gridDim.x * 256) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(B[c]) & 0x7fffffffffffffffull;
        if (bits > mx) mx = bits;
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d && red[threadIdx.x + d] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(max_bits, red[0]);
}

__global__ void __launch_bounds__(256) msnv_pcoa_diag_k(const double *__restrict__ A, uint32_t n, double *__restrict__ diag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) diag[i] = A[(size_t)i * n + i];
}

__global__ void __launch_bounds__(PAIR_THREADS) msnv_pcoa_params_k(const double *__restrict__ A, uint32_t n, uint32_t m, uint32_t r, double tol,
                                                                   Rot *__restrict__ rot, uint32_t *__restrict__ n_rotations) {
    const uint32_t i = blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (i >= m / 2) return;
    uint32_t p, q;
    pair_of(m, r, i, p, q);
    Rot R{1.0, 0.0, 0.0, 0, 0};
    if (q < n) {
        const double apq = A[(size_t)p * n + q];
        if (fabs(apq) > tol) {
            const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
            const double theta = (aqq - app) / (2.0 * apq);
            R.t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            R.c = 1.0 / sqrt(R.t * R.t + 1.0);
            R.s = R.t * R.c;
            R.rotates = 1;
            atomicAdd(n_rotations, 1u);
        }
    }
    rot[i] = R;
}

__global__ void __launch_bounds__(ROT_X *ROT_Y) msnv_pcoa_rotate_k(double *__restrict__ A, double *__restrict__ V, uint32_t n, uint32_t m, uint32_t r,
                                                                    const Rot *__restrict__ rot) {
    const uint32_t h = m / 2, J = blockIdx.x * ROT_X + threadIdx.x, y = blockIdx.y * ROT_Y + threadIdx.y;
    if (J >= h || y >= h + n) return;
    uint32_t pj, qj;
    pair_of(m, r, J, pj, qj);
    const Rot RJ = rot[J];
    if (y >= h) {                                                      // a row of V: the column form alone
        if (qj >= n) return;
        double *row = V + (size_t)(y - h) * n;
        const double x = row[pj], z = row[qj];
        row[pj] = RJ.c * x - RJ.s * z;
        row[qj] = RJ.s * x + RJ.c * z;
        return;
    }
    const uint32_t I = y;
    if (I > J) return;
    uint32_t pi, qi;
    pair_of(m, r, I, pi, qi);
    if (I == J) {                                                      // the pair's own block
        if (qi >= n) return;
        const double apq = A[(size_t)pi * n + qi];
        A[(size_t)pi * n + pi] = A[(size_t)pi * n + pi] - RJ.t * apq;
        A[(size_t)qi * n + qi] = A[(size_t)qi * n + qi] + RJ.t * apq;
        if (RJ.rotates) { A[(size_t)pi * n + qi] = 0.0; A[(size_t)qi * n + pi] = 0.0; }
        return;
    }
    // I < J: J is not slot 0, so it is a full pair; I may be the bye
    const double w = A[(size_t)pi * n + pj], x = A[(size_t)pi * n + qj];
    const double w1 = RJ.c * w - RJ.s * x, x1 = RJ.s * w + RJ.c * x;
    if (qi >= n) {
        A[(size_t)pi * n + pj] = w1; A[(size_t)pj * n + pi] = w1;
        A[(size_t)pi * n + qj] = x1; A[(size_t)qj * n + pi] = x1;
        return;
    }
    const Rot RI = rot[I];
    const double yy = A[(size_t)qi * n + pj], z = A[(size_t)qi * n + qj];
    const double y1 = RJ.c * yy - RJ.s * z, z1 = RJ.s * yy + RJ.c * z;
    const double w2 = RI.c * w1 - RI.s * y1, y2 = RI.s * w1 + RI.c * y1;
    const double x2 = RI.c * x1 - RI.s * z1, z2 = RI.s * x1 + RI.c * z1;
    A[(size_t)pi * n + pj] = w2; A[(size_t)pj * n + pi] = w2;
    A[(size_t)pi * n + qj] = x2; A[(size_t)qj * n + pi] = x2;
    A[(size_t)qi * n + pj] = y2; A[(size_t)pj * n + qi] = y2;
    A[(size_t)qi * n + qj] = z2; A[(size_t)qj * n + qi] = z2;
}

// axis a < k: column col[a] of V times sqrt(lam[a]), negated when the column's first component of largest magnitude is negative; a >= k: NaN
__global__ void __launch_bounds__(AXIS_THREADS) msnv_pcoa_axes_k(const double *__restrict__ V, uint32_t n, uint32_t n_axes, uint32_t k, const uint32_t *__restrict__ col,
                                                                 const double *__restrict__ lam, double *__restrict__ out) {
    __shared__ double red_v[AXIS_THREADS];
    __shared__ uint32_t red_i[AXIS_THREADS];
    const uint32_t a = blockIdx.x, tid = threadIdx.x;
    if (a >= k) {
        for (uint32_t i = tid; i < n; i += AXIS_THREADS) out[(size_t)i * n_axes + a] = __longlong_as_double((long long)NAN_BITS);
        return;
    }
    const double *v = V + col[a];
    double bv = -1.0;
    uint32_t bi = 0xffffffffu;
    for (uint32_t i = tid; i < n; i += AXIS_THREADS) {
        const double x = fabs(v[(size_t)i * n]);
        if (x > bv) { bv = x; bi = i; }                                // ascending i inside the lane: the first of equals stays
    }
    red_v[tid] = bv; red_i[tid] = bi;
    __syncthreads();
    for (uint32_t d = AXIS_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) {
            const double ov = red_v[tid + d];
            const uint32_t oi = red_i[tid + d];
            if (ov > red_v[tid] || (ov == red_v[tid] && oi < red_i[tid])) { red_v[tid] = ov; red_i[tid] = oi; }
        }
        __syncthreads();
    }
    const bool flip = v[(size_t)red_i[0] * n] < 0.0;
    const double scale = sqrt(lam[a]);
    for (uint32_t i = tid; i < n; i += AXIS_THREADS) {
        const double x = v[(size_t)i * n] * scale;
        out[(size_t)i * n_axes + a] = flip ? -x : x;
    }
}

// ---------------------------------------------------------------------------------------------- host side of the launches
int dev_pcoa(const char *who, const double *dist, uint32_t n, uint32_t n_axes, void *stream, double *eig, double *rel_eig, double *axis_pct, double *vectors,
             int64_t info[8], double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t m = n + (n & 1), h = m / 2;
    const size_t cells = (size_t)n * n;
    Buf d_dist, d_a, d_v, d_mean, d_diag, d_rot, d_word, d_col, d_lam, d_out;
    MSNV_TRY(d_dist.upload(dist, cells * 8, st));
    MSNV_TRY(d_a.alloc(cells * 8));
    MSNV_TRY(d_v.alloc(cells * 8));
    MSNV_TRY(d_mean.alloc((size_t)(n + 1) * 8));
    MSNV_TRY(d_diag.alloc((size_t)n * 8));
    MSNV_TRY(d_rot.alloc((size_t)h * sizeof(Rot)));
    MSNV_TRY(d_word.alloc(16));                                        // [0] the bits of max |B_ij| (64-bit) [2] rotating pairs so far (32-bit)
    HIP_TRY(hipMemsetAsync(d_word.p, 0, 16, st));
    unsigned long long *d_max = d_word.as<unsigned long long>();
    uint32_t *d_cnt = d_word.as<uint32_t>() + 2;
    KernelTimer tm;

    // ---- Gower centring, V = I, tol
    const dim3 tile(ROT_X, ROT_Y);
    MSNV_TRY(tm.begin(st));
    hipLaunchKernelGGL(msnv_pcoa_rowmean_k, dim3((n + 255) / 256), dim3(256), 0, st, d_dist.as<double>(), n, d_mean.as<double>());
    hipLaunchKernelGGL(msnv_pcoa_grand_k, dim3(1), dim3(64), 0, st, d_mean.as<double>(), n);
    hipLaunchKernelGGL(msnv_pcoa_centre_k, dim3((n + ROT_X - 1) / ROT_X, (n + ROT_Y - 1) / ROT_Y), tile, 0, st, d_dist.as<double>(), n, d_mean.as<double>(), d_a.as<double>(),
                       d_v.as<double>());
    hipLaunchKernelGGL(msnv_pcoa_absmax_k, dim3((uint32_t)std::min<size_t>((cells + 255) / 256, dev_resident_workgroups(8))), dim3(256), 0, st, d_a.as<double>(),
                       (unsigned long long)cells, d_max);
    hipLaunchKernelGGL(msnv_pcoa_diag_k, dim3((n + 255) / 256), dim3(256), 0, st, d_a.as<double>(), n, d_diag.as<double>());
    MSNV_TRY(tm.stop(st));
    unsigned long long max_bits = 0;
    std::vector<double> diag(n);
    HIP_TRY(hipMemcpyAsync(&max_bits, d_max, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(diag.data(), d_diag.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    if (max_bits >= INF_BITS) return fail(MSNV_EDOMAIN, "%s: the squared distances of %u samples overflow", who, n);
    double max_abs, trace = 0.0;
    memcpy(&max_abs, &max_bits, 8);
    const double tol = 0x1p-52 * max_abs;
    for (uint32_t i = 0; i < n; ++i) trace += diag[i];

    // ---- sweeps: 2 (m - 1) launches each, then one wait for the counter
    const dim3 rot_grid((h + ROT_X - 1) / ROT_X, (h + n + ROT_Y - 1) / ROT_Y);
    uint32_t sweeps = 0, rotations = 0;
    bool settled = false;
    while (!settled && sweeps < PCOA_MAX_SWEEPS) {
        MSNV_TRY(tm.begin(st));
        for (uint32_t r = 0; r + 1 < m; ++r) {
            hipLaunchKernelGGL(msnv_pcoa_params_k, dim3((h + PAIR_THREADS - 1) / PAIR_THREADS), dim3(PAIR_THREADS), 0, st, d_a.as<double>(), n, m, r, tol, d_rot.as<Rot>(), d_cnt);
            hipLaunchKernelGGL(msnv_pcoa_rotate_k, rot_grid, tile, 0, st, d_a.as<double>(), d_v.as<double>(), n, m, r, d_rot.as<Rot>());
        }
        MSNV_TRY(tm.stop(st));
        uint32_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, d_cnt, 4, hipMemcpyDeviceToHost, st));
        MSNV_TRY(tm.wait(st));
        ++sweeps;
        settled = total == rotations;
        rotations = total;
    }
    if (!settled) return fail(MSNV_EDOMAIN, "%s: the Jacobi solve of %u samples has not settled after %u sweeps", who, n, sweeps);

    // ---- the n eigenvalues on the host: order, cut-off, shares
    MSNV_TRY(tm.begin(st));
    hipLaunchKernelGGL(msnv_pcoa_diag_k, dim3((n + 255) / 256), dim3(256), 0, st, d_a.as<double>(), n, d_diag.as<double>());
    MSNV_TRY(tm.stop(st));
    HIP_TRY(hipMemcpyAsync(diag.data(), d_diag.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return diag[x] > diag[y]; });
    const double cut = sqrt(0x1p-52);
    uint32_t k = 0, n_neg = 0;
    double pos_sum = 0.0;
    for (uint32_t a = 0; a < n; ++a) {
        const double l = diag[order[a]];
        eig[a] = fabs(l) < cut ? 0.0 : l;
        k += eig[a] > cut; n_neg += eig[a] < -cut;
        pos_sum += eig[a] > 0.0 ? eig[a] : 0.0;
    }
    for (uint32_t a = 0; a < n; ++a) {
        rel_eig[a] = eig[a] / trace;
        axis_pct[a] = (eig[a] > 0.0 ? eig[a] : 0.0) / pos_sum * 100.0;
    }

    // ---- the axes
    MSNV_TRY(d_col.upload(order.data(), (size_t)n_axes * 4, st));
    MSNV_TRY(d_lam.upload(eig, (size_t)n_axes * 8, st));
    MSNV_TRY(d_out.alloc((size_t)n * n_axes * 8));
    MSNV_TRY(tm.begin(st));
    hipLaunchKernelGGL(msnv_pcoa_axes_k, dim3(n_axes), dim3(AXIS_THREADS), 0, st, d_v.as<double>(), n, n_axes, k, d_col.as<uint32_t>(), d_lam.as<double>(), d_out.as<double>());
    MSNV_TRY(tm.stop(st));
    HIP_TRY(hipMemcpyAsync(vectors, d_out.p, (size_t)n * n_axes * 8, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    info[0] = k < 2 ? MSNV_PCOA_TOO_FEW_AXES : MSNV_PCOA_OK;
    info[1] = sweeps; info[2] = rotations; info[3] = k; info[4] = n_neg; info[5] = info[6] = info[7] = 0;
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
