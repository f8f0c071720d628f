// metasnv_amd/csrc/cluster_k.hip -- subpopr's clustering arithmetic on the device (src/subpopr/R/clustering.R; the host side is cluster.cpp).
//
//   msnv_pam_tasks_k     cluster::pam(diss = TRUE, pamonce = 0) of many index subsets of one resident distance matrix: one workgroup per task
//   msnv_ps_splits_k     predStrengthCustom's tail (:176-201) of many splits: classify each half by the other half's medoids, count the
//                        co-classified pairs, prederr = (min ps[1,] + min ps[2,]) / 2; one workgroup per split
//   msnv_freq_bands_k    computeSnvFreqStats (computeSnvFreqStats.R:1-24): per sample column, cells outside 20/80, 10/90, 5/95 and cells that count
//   msnv_boot_match_k    fpc::clusterboot(bootmethod = "subset")'s comparison (clusteringStability.R:129-148): per re-clustered subset, the contingency
//                        table of (original cluster, new cluster) and each original cluster's best Jaccard pair; one workgroup per subset
//
// One route.  A task's m x m sub-matrix is never gathered: d(i, j) is read from the full n x n matrix through the task's index list, as
// D[col[j] * n + col[i]] -- the matrix is symmetric, so the lanes of a wavefront (different i or h, the same j) read one row of it.  At the
// stage's sizes (n of a few hundred) the whole matrix sits in L2, and no scratch bounds the number of tasks in flight (KERNELS.md).
// Parallelism: BUILD has one lane per candidate i, SWAP one lane per (h, i) pair; the loop over j is inside the lane, ascending, so every sum
// is the sequential fp64 sum the rules name (include/msnv.h).  Arg-max / arg-min across lanes compare (value, index) pairs: BUILD keeps the
// LAST largest, SWAP the FIRST smallest in (h ascending, i ascending) order -- what the sequential loops would keep.
// LDS per workgroup (dynamic, sized by the largest task of the launch): dysma[m] dysmb[m] f64 | col[m] ismed[m] med[k] u32 = 28 bytes per member.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

#pragma clang fp contract(off)

namespace msnv {

namespace {

constexpr uint32_t PAM_THREADS = 256;

struct PamTask { unsigned long long off, med_off; uint32_t m, k; };      // its list in idx / cluster, its medoids in the medoid output

struct Best { double v; uint32_t key; };

// The winner over the workgroup, the same in every thread.  LAST: larger value, then larger key; else smaller value, then smaller key.
template <bool LAST> __device__ inline Best block_best(Best b, double *red_v, uint32_t *red_k) {
    red_v[threadIdx.x] = b.v; red_k[threadIdx.x] = b.key;
    __syncthreads();
    for (uint32_t d = PAM_THREADS / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const double ov = red_v[threadIdx.x + d], mv = red_v[threadIdx.x];
            const uint32_t ok = red_k[threadIdx.x + d], mk = red_k[threadIdx.x];
            const bool take = LAST ? (ov > mv || (ov == mv && ok > mk)) : (ov < mv || (ov == mv && ok < mk));
            if (take) { red_v[threadIdx.x] = ov; red_k[threadIdx.x] = ok; }
        }
        __syncthreads();
    }
    Best r{red_v[0], red_k[0]};
    __syncthreads();
    return r;
}

}  // namespace

__global__ void __launch_bounds__(PAM_THREADS) msnv_pam_tasks_k(const double *__restrict__ D, uint32_t n, const PamTask *__restrict__ tasks, unsigned long long n_tasks,
                                                                const int32_t *__restrict__ idx, uint32_t lds_m, int32_t *__restrict__ med_out,
                                                                int32_t *__restrict__ clus_out, int32_t *__restrict__ swaps_out, uint32_t *__restrict__ err) {
    extern __shared__ unsigned char pam_lds[];
    __shared__ double red_v[PAM_THREADS];
    __shared__ uint32_t red_k[PAM_THREADS];
    __shared__ double s_sky;
    double *dysma = (double *)pam_lds, *dysmb = dysma + lds_m;
    uint32_t *col = (uint32_t *)(dysmb + lds_m), *ismed = col + lds_m, *med = ismed + lds_m;
    const uint32_t tid = threadIdx.x;
    for (unsigned long long t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const PamTask T = tasks[t];
        const uint32_t m = T.m, k = T.k;
        __syncthreads();                                               // the task before is done with the LDS
        for (uint32_t j = tid; j < m; j += PAM_THREADS) { col[j] = (uint32_t)idx[T.off + j]; ismed[j] = 0; }
        __syncthreads();
        // ---- BUILD
        Best mx{0.0, 0};
        for (uint32_t p = tid; p < m * m; p += PAM_THREADS) {
            const double d = D[(size_t)col[p / m] * n + col[p % m]];
            if (d > mx.v) mx.v = d;
        }
        mx = block_best<true>(mx, red_v, red_k);
        const double s = 1.1 * mx.v + 1.0;
        for (uint32_t j = tid; j < m; j += PAM_THREADS) dysma[j] = s;
        __syncthreads();
        for (uint32_t step = 0; step < k; ++step) {
            Best b{-1.0, 0};
            for (uint32_t i = tid; i < m; i += PAM_THREADS) {
                if (ismed[i]) continue;
                const uint32_t ci = col[i];
                double beter = 0.0;
                for (uint32_t j = 0; j < m; ++j) {
                    const double cmd = dysma[j] - D[(size_t)col[j] * n + ci];
                    if (cmd > 0.0) beter += cmd;
                }
                if (beter >= b.v) { b.v = beter; b.key = i; }
            }
            b = block_best<true>(b, red_v, red_k);
            const uint32_t ci = col[b.key];
            for (uint32_t j = tid; j < m; j += PAM_THREADS) {
                const double d = D[(size_t)col[j] * n + ci];
                if (dysma[j] > d) dysma[j] = d;
            }
            if (tid == 0) ismed[b.key] = 1;
            __syncthreads();
        }
        if (tid == 0) {
            double sky = 0.0;
            uint32_t c = 0;
            for (uint32_t j = 0; j < m; ++j) { sky += dysma[j]; if (ismed[j]) med[c++] = j; }
            s_sky = sky;
        }
        __syncthreads();
        // ---- SWAP
        uint32_t n_swaps = 0;
        while (k > 1) {
            for (uint32_t j = tid; j < m; j += PAM_THREADS) {
                const uint32_t cj = col[j];
                double a = s, b = s;
                for (uint32_t c = 0; c < k; ++c) {
                    const double d = D[(size_t)col[med[c]] * n + cj];
                    if (a > d) { b = a; a = d; } else if (b > d) b = d;
                }
                dysma[j] = a; dysmb[j] = b;
            }
            __syncthreads();
            Best b{1.0, 0xffffffffu};
            for (uint32_t p = tid; p < m * k; p += PAM_THREADS) {
                const uint32_t h = p / k;
                if (ismed[h]) continue;
                const uint32_t ch = col[h], ci = col[med[p % k]];
                double dz = 0.0;
                for (uint32_t j = 0; j < m; ++j) {
                    const double *row = D + (size_t)col[j] * n;
                    const double hj = row[ch], ij = row[ci], a = dysma[j];
                    if (ij == a) {
                        const double bb = dysmb[j], small = bb > hj ? hj : bb;
                        dz += small - a;
                    } else if (hj < a) dz += hj - a;
                }
                if (dz < b.v) { b.v = dz; b.key = p; }
            }
            b = block_best<false>(b, red_v, red_k);
            const double sky = s_sky;
            if (!(b.v < -16.0 * DBL_EPSILON * fabs(sky))) break;
            if (++n_swaps > PAM_MAX_SWAPS) { if (tid == 0) atomicOr(err, 1u); break; }
            __syncthreads();                                           // every thread has read s_sky and the old medoids
            if (tid == 0) {
                const uint32_t h = b.key / k;
                uint32_t c = b.key % k;
                ismed[med[c]] = 0; ismed[h] = 1;
                for (; c + 1 < k && med[c + 1] < h; ++c) med[c] = med[c + 1];       // med[] stays ascending
                for (; c > 0 && med[c - 1] > h; --c) med[c] = med[c - 1];
                med[c] = h;
                s_sky = sky + b.v;
            }
            __syncthreads();
        }
        // ---- every member to its nearest medoid
        for (uint32_t j = tid; j < m; j += PAM_THREADS) {
            const uint32_t cj = col[j];
            double best = D[(size_t)col[med[0]] * n + cj];
            uint32_t cl = 0;
            for (uint32_t c = 1; c < k; ++c) {
                const double d = D[(size_t)col[med[c]] * n + cj];
                if (d < best) { best = d; cl = c; }
            }
            clus_out[T.off + j] = (int32_t)cl + 1;
        }
        for (uint32_t c = tid; c < k; c += PAM_THREADS) med_out[T.med_off + c] = (int32_t)med[c];
        if (tid == 0) swaps_out[t] = (int32_t)n_swaps;
    }
}

// LDS (dynamic): cls[L] | pairs[2k] nik[2k] alen[2k], u32.  Everything it counts is an integer, so the atomics' order does not matter.
__global__ void __launch_bounds__(PAM_THREADS) msnv_ps_splits_k(const double *__restrict__ D, uint32_t n, const PamTask *__restrict__ tasks,
                                                                unsigned long long n_splits, const int32_t *__restrict__ idx, uint32_t lds_len, const int32_t *__restrict__ med,
                                                                const int32_t *__restrict__ clus, double *__restrict__ prederr) {
    extern __shared__ unsigned char ps_lds[];
    uint32_t *cls = (uint32_t *)ps_lds, *cnt = cls + lds_len;
    const uint32_t tid = threadIdx.x;
    for (unsigned long long s = blockIdx.x; s < n_splits; s += gridDim.x) {
        const PamTask H0 = tasks[2 * s], H1 = tasks[2 * s + 1];    // a split's halves are two tasks with adjacent lists
        const uint32_t k = H0.k, L = H0.m + H1.m;
        uint32_t *pairs = cnt, *nik = cnt + 2 * k, *alen = cnt + 4 * k;
        __syncthreads();
        for (uint32_t c = tid; c < 6 * k; c += PAM_THREADS) cnt[c] = 0;
        for (uint32_t t = tid; t < L; t += PAM_THREADS) {              // classifdist(method = "centroid"): which.min over the other half's medoids
            const PamTask &O = t < H0.m ? H1 : H0;
            const uint32_t ct = (uint32_t)idx[H0.off + t];
            double best = 0.0;
            uint32_t cl = 0;
            for (uint32_t c = 0; c < k; ++c) {
                const double d = D[(size_t)idx[O.off + med[O.med_off + c]] * n + ct];
                if (c == 0 || d < best) { best = d; cl = c; }
            }
            cls[t] = cl;
        }
        __syncthreads();
        for (uint32_t t = tid; t < L; t += PAM_THREADS) {
            const uint32_t h = t < H0.m ? 0 : 1, lo = h ? H0.m : 0, mh = h ? H1.m : H0.m;
            const uint32_t kk = (uint32_t)clus[H0.off + t] - 1;
            atomicAdd(&nik[h * k + kk], 1u);
            if (t - lo >= mh - 1) continue;                            // the half's last entry is left out of the numerator (:191)
            uint32_t same = 0;
            for (uint32_t u = lo; u < lo + mh - 1; ++u) same += ((uint32_t)clus[H0.off + u] - 1 == kk && cls[u] == cls[t]) ? 1u : 0u;
            atomicAdd(&alen[h * k + kk], 1u);
            atomicAdd(&pairs[h * k + kk], same);
        }
        __syncthreads();
        if (tid == 0) {
            double mn[2];
            for (uint32_t h = 0; h < 2; ++h)
                for (uint32_t kk = 0; kk < k; ++kk) {
                    const uint32_t nk = nik[h * k + kk];
                    const double ps = nk > 1 ? (double)(pairs[h * k + kk] - alen[h * k + kk]) / (double)(nk * (nk - 1)) : 0.0;
                    if (kk == 0 || ps < mn[h]) mn[h] = ps;
                }
            prederr[s] = (mn[0] + mn[1]) / 2.0;
        }
    }
}

// Task 0 is the original partition (its list = the members), task s + 1 re-clusters subset s; pos holds, packed in the subsets' order, each entry's
// position in task 0's list.  Per subset: tab[j][c] = entries in original cluster j and new cluster c (LDS atomics on integers: their order does
// not matter), row and column sums, then one lane per original cluster walks the new clusters in ascending order and keeps the FIRST largest
// inter / union, compared as inter * best_union > best_inter * union (at most 4096 * 8192, inside 32 bits).  A new cluster without a member (its
// medoid is a duplicate of an earlier one) is passed over, so a union is never 0.  best[(s * k + j) * 2] = inter, + 1 = union.
// A workgroup per subset, not a wavefront: a subset has up to 4096 entries (16 per lane here, 64 per lane of one wavefront), the PAM launch before
// it is shaped the same way, and the statics are one table per workgroup with no bookkeeping of which wavefront owns which slice.
__global__ void __launch_bounds__(PAM_THREADS) msnv_boot_match_k(const PamTask *__restrict__ tasks, unsigned long long n_sets, const int32_t *__restrict__ pos,
                                                                 const int32_t *__restrict__ clus, int32_t *__restrict__ best) {
    __shared__ uint32_t tab[CLUSTER_BOOT_MAX_K * CLUSTER_BOOT_MAX_K], rowsum[CLUSTER_BOOT_MAX_K], colsum[CLUSTER_BOOT_MAX_K];
    const uint32_t tid = threadIdx.x;
    const PamTask O = tasks[0];
    const uint32_t k = O.k;
    for (unsigned long long s = blockIdx.x; s < n_sets; s += gridDim.x) {
        const PamTask T = tasks[s + 1];
        __syncthreads();                                               // the subset before is done with the table
        for (uint32_t c = tid; c < k * k; c += PAM_THREADS) tab[c] = 0;
        __syncthreads();
        for (uint32_t e = tid; e < T.m; e += PAM_THREADS) {
            const uint32_t j = (uint32_t)clus[O.off + (uint32_t)pos[T.off - O.m + e]] - 1, c = (uint32_t)clus[T.off + e] - 1;
            atomicAdd(&tab[j * k + c], 1u);
        }
        __syncthreads();
        if (tid < k) {
            uint32_t r = 0, cs = 0;
            for (uint32_t c = 0; c < k; ++c) { r += tab[tid * k + c]; cs += tab[c * k + tid]; }
            rowsum[tid] = r; colsum[tid] = cs;
        }
        __syncthreads();
        if (tid < k) {
            uint32_t bi = 0, bu = 0;
            for (uint32_t c = 0; c < k; ++c) {
                if (colsum[c] == 0) continue;
                const uint32_t inter = tab[tid * k + c], uni = rowsum[tid] + colsum[c] - inter;
                if (bu == 0 || inter * bu > bi * uni) { bi = inter; bu = uni; }
            }
            best[(s * k + tid) * 2] = (int32_t)bi; best[(s * k + tid) * 2 + 1] = (int32_t)bu;
        }
    }
}

// counts[sample][4]: cells < 20 or > 80, < 10 or > 90, < 5 or > 95, cells that count (not NaN: read_freq turns -1 and NA into NaN).
// A thread per sample column, a block row per FREQ_ROWS positions: the lanes of a wavefront read one table row.
constexpr uint32_t FREQ_ROWS = 512;
__global__ void __launch_bounds__(256) msnv_freq_bands_k(const double *__restrict__ rows, unsigned long long n_pos, uint32_t S, unsigned long long *__restrict__ counts) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const unsigned long long p0 = (unsigned long long)blockIdx.y * FREQ_ROWS, p1 = p0 + FREQ_ROWS < n_pos ? p0 + FREQ_ROWS : n_pos;
    unsigned long long c20 = 0, c10 = 0, c5 = 0, ok = 0;
    for (unsigned long long p = p0; p < p1; ++p) {
        const double x = rows[p * S + s];
        if (x != x) continue;
        ++ok;
        c20 += (x < 20.0 || x > 80.0) ? 1 : 0;
        c10 += (x < 10.0 || x > 90.0) ? 1 : 0;
        c5 += (x < 5.0 || x > 95.0) ? 1 : 0;
    }
    atomicAdd(&counts[(size_t)s * 4 + 0], c20); atomicAdd(&counts[(size_t)s * 4 + 1], c10);
    atomicAdd(&counts[(size_t)s * 4 + 2], c5); atomicAdd(&counts[(size_t)s * 4 + 3], ok);
}

// ---------------------------------------------------------------------------------------------- host side of the launches
namespace {

constexpr uint64_t BATCH_ENTRIES = 1ull << 26;                         // list entries of one launch: 256 MiB of indices, as much of cluster ids

// msnv_cluster_boot's second launch: the batch is task 0 = the original partition and one task per subset (the whole batch, never a part of one)
struct Boot { const int32_t *pos; int32_t *med0, *clus0, *best; };

// One launch of the PAM kernel over tasks[t0, t1) (their offsets rebased to the batch) and, when splits are asked for, one of the tail kernel; with
// boot, one of the matching kernel over the cluster ids the PAM kernel left on the device.
int run_batch(const ClusterDev &c, const std::vector<PamTask> &tasks, uint64_t t0, uint64_t t1, const int32_t *idx, bool splits, hipStream_t st,
              int32_t *med, int32_t *clus, int32_t *swaps, double *prederr, KernelTimer &tm, const Boot *boot = nullptr) {
    const uint64_t nt = t1 - t0, off0 = tasks[t0].off, med0 = tasks[t0].med_off;
    const uint64_t n_idx = tasks[t1 - 1].off + tasks[t1 - 1].m - off0, n_med = tasks[t1 - 1].med_off + tasks[t1 - 1].k - med0;
    std::vector<PamTask> local(tasks.begin() + t0, tasks.begin() + t1);
    uint32_t max_m = 0, max_len = 0, max_k = 0;
    for (uint64_t t = 0; t < nt; ++t) {
        local[t].off -= off0; local[t].med_off -= med0;
        max_m = std::max(max_m, local[t].m); max_k = std::max(max_k, local[t].k);
        if (splits && !(t & 1)) max_len = std::max(max_len, local[t].m + local[t + 1].m);
    }
    const uint64_t ns = splits ? nt / 2 : 0;
    Buf d_tasks, d_idx, d_med, d_clus, d_swaps, d_err, d_pe, d_pos, d_best;
    MSNV_TRY(d_tasks.upload(local.data(), nt * sizeof(PamTask), st));
    MSNV_TRY(d_idx.upload(idx + off0, n_idx * 4, st));
    MSNV_TRY(d_med.alloc(n_med * 4));
    MSNV_TRY(d_clus.alloc(n_idx * 4));
    MSNV_TRY(d_swaps.alloc(nt * 4));
    MSNV_TRY(d_err.alloc(16));
    HIP_TRY(hipMemsetAsync(d_err.p, 0, 16, st));
    if (ns) MSNV_TRY(d_pe.alloc(ns * 8));
    const uint64_t n_sets = boot ? nt - 1 : 0, n_pos = boot ? n_idx - local[0].m : 0, n_best = n_sets * max_k * 2;
    if (n_sets) {
        MSNV_TRY(d_pos.upload(boot->pos, n_pos * 4, st));
        MSNV_TRY(d_best.alloc(n_best * 4));
    }
    const size_t lds_pam = (size_t)max_m * 28, lds_ps = (size_t)max_len * 4 + (size_t)max_k * 24;
    if (lds_pam > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)msnv_pam_tasks_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pam));
    if (lds_ps > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)msnv_ps_splits_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ps));
    const uint32_t per_cu = (uint32_t)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (lds_pam + 4096)));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nt, dev_resident_workgroups(per_cu));
    MSNV_TRY(tm.begin(st));
    hipLaunchKernelGGL(msnv_pam_tasks_k, dim3(grid), dim3(PAM_THREADS), lds_pam, st, c.dist, c.n, d_tasks.as<PamTask>(), (unsigned long long)nt, d_idx.as<int32_t>(), max_m,
                       d_med.as<int32_t>(), d_clus.as<int32_t>(), d_swaps.as<int32_t>(), d_err.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (ns) {
        hipLaunchKernelGGL(msnv_ps_splits_k, dim3((uint32_t)std::min<uint64_t>(ns, dev_resident_workgroups(8))), dim3(PAM_THREADS), lds_ps, st, c.dist, c.n, d_tasks.as<PamTask>(),
                           (unsigned long long)ns, d_idx.as<int32_t>(), max_len, d_med.as<int32_t>(), d_clus.as<int32_t>(), d_pe.as<double>());
        HIP_TRY(hipGetLastError());
    }
    if (n_sets)
        hipLaunchKernelGGL(msnv_boot_match_k, dim3((uint32_t)std::min<uint64_t>(n_sets, dev_resident_workgroups(8))), dim3(PAM_THREADS), 0, st, d_tasks.as<PamTask>(),
                           (unsigned long long)n_sets, d_pos.as<int32_t>(), d_clus.as<int32_t>(), d_best.as<int32_t>());
    MSNV_TRY(tm.stop(st));
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, st));
    if (boot) {
        HIP_TRY(hipMemcpyAsync(boot->med0, d_med.p, (size_t)local[0].k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(boot->clus0, d_clus.p, (size_t)local[0].m * 4, hipMemcpyDeviceToHost, st));
        if (n_sets) HIP_TRY(hipMemcpyAsync(boot->best, d_best.p, n_best * 4, hipMemcpyDeviceToHost, st));
    }
    if (med) HIP_TRY(hipMemcpyAsync(med + med0, d_med.p, n_med * 4, hipMemcpyDeviceToHost, st));
    if (clus) HIP_TRY(hipMemcpyAsync(clus + off0, d_clus.p, n_idx * 4, hipMemcpyDeviceToHost, st));
    if (swaps) HIP_TRY(hipMemcpyAsync(swaps + t0, d_swaps.p, nt * 4, hipMemcpyDeviceToHost, st));
    if (prederr) HIP_TRY(hipMemcpyAsync(prederr + t0 / 2, d_pe.p, ns * 8, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    if (err) return fail(MSNV_EDOMAIN, "PAM: a task swapped more than %u times without settling", PAM_MAX_SWAPS);
    return MSNV_OK;
}

// tasks in launches of at most BATCH_ENTRIES list entries (a split's two halves stay together)
int run_all(const ClusterDev &c, const std::vector<PamTask> &tasks, const int32_t *idx, bool splits, void *stream, int32_t *med, int32_t *clus, int32_t *swaps,
            double *prederr, double *ms_kernel) {
    KernelTimer tm;
    const uint64_t step = splits ? 2 : 1;
    for (uint64_t t0 = 0; t0 < tasks.size();) {
        uint64_t t1 = t0 + step;
        while (t1 < tasks.size() && tasks[t1 + step - 1].off + tasks[t1 + step - 1].m - tasks[t0].off <= BATCH_ENTRIES) t1 += step;
        MSNV_TRY(run_batch(c, tasks, t0, t1, idx, splits, (hipStream_t)stream, med, clus, swaps, prederr, tm));
        t0 = t1;
    }
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace

ClusterDev::~ClusterDev() { if (dist) (void)hipFree(dist); }

int dev_cluster_upload(ClusterDev &c, const double *dist, uint32_t n, void *stream) {
    if (c.dist) { (void)hipFree(c.dist); c.dist = nullptr; }
    HIP_TRY(hipMalloc((void **)&c.dist, (size_t)n * n * 8));
    c.n = n;
    HIP_TRY(hipMemcpyAsync(c.dist, dist, (size_t)n * n * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MSNV_OK;
}

int dev_pam_tasks(const ClusterDev &c, uint64_t n_tasks, const uint32_t *m, const uint32_t *k, const int32_t *idx, void *stream, int32_t *med, int32_t *clus,
                  int32_t *swaps, double *ms_kernel) {
    std::vector<PamTask> tasks(n_tasks);
    uint64_t off = 0, med_off = 0;
    for (uint64_t t = 0; t < n_tasks; ++t) { tasks[t] = PamTask{off, med_off, m[t], k[t]}; off += m[t]; med_off += k[t]; }
    return run_all(c, tasks, idx, false, stream, med, clus, swaps, nullptr, ms_kernel);
}

int dev_cluster_boot(const ClusterDev &c, uint64_t n_sets, const uint32_t *m, uint32_t k, const int32_t *idx, const int32_t *pos, void *stream, int32_t *med0,
                     int32_t *clus0, int32_t *best, double *ms_kernel) {
    std::vector<PamTask> tasks(n_sets + 1);
    uint64_t off = 0;
    for (uint64_t t = 0; t <= n_sets; ++t) { tasks[t] = PamTask{off, t * k, m[t], k}; off += m[t]; }
    if (off > BATCH_ENTRIES) return fail(MSNV_ECAPACITY, "cluster boot: %llu list entries in one call (at most %llu)", (unsigned long long)off, (unsigned long long)BATCH_ENTRIES);
    const Boot boot{pos, med0, clus0, best};
    KernelTimer tm;
    MSNV_TRY(run_batch(c, tasks, 0, tasks.size(), idx, false, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr, tm, &boot));
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

int dev_pred_strength(const ClusterDev &c, uint64_t n_splits, const uint32_t *len, const uint32_t *k, const int32_t *idx, void *stream, double *prederr, double *ms_kernel) {
    std::vector<PamTask> tasks(2 * n_splits);
    uint64_t off = 0, med_off = 0;
    for (uint64_t s = 0; s < n_splits; ++s) {
        const uint32_t m0 = len[s] / 2, m1 = len[s] - m0;
        tasks[2 * s] = PamTask{off, med_off, m0, k[s]};
        tasks[2 * s + 1] = PamTask{off + m0, med_off + k[s], m1, k[s]};
        off += len[s]; med_off += 2ull * k[s];
    }
    return run_all(c, tasks, idx, true, stream, nullptr, nullptr, nullptr, prederr, ms_kernel);
}

int dev_freq_bands(const double *rows, uint64_t n_pos, uint32_t S, void *stream_, uint64_t *counts, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    Buf d_rows, d_cnt;
    MSNV_TRY(d_cnt.alloc((size_t)S * 32));
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, (size_t)S * 32, st));
    // position chunks that fit the device and the grid's second dimension
    const uint64_t row_bytes = (uint64_t)S * 8;
    uint64_t chunk = 0;
    MSNV_TRY(slab_rows(n_pos, row_bytes, 0.5, (uint64_t)FREQ_ROWS * 65535, "SNV frequency composition", &chunk));
    MSNV_TRY(d_rows.alloc(chunk * row_bytes));
    KernelTimer tm;
    for (uint64_t p0 = 0; p0 < n_pos; p0 += chunk) {
        const uint64_t np = std::min(chunk, n_pos - p0);
        HIP_TRY(hipMemcpyAsync(d_rows.p, rows + p0 * S, np * row_bytes, hipMemcpyHostToDevice, st));
        MSNV_TRY(tm.begin(st));
        hipLaunchKernelGGL(msnv_freq_bands_k, dim3((S + 255) / 256, (uint32_t)((np + FREQ_ROWS - 1) / FREQ_ROWS)), dim3(256), 0, st, d_rows.as<double>(), (unsigned long long)np, S,
                           d_cnt.as<unsigned long long>());
        MSNV_TRY(tm.end(st));
    }
    HIP_TRY(hipMemcpy(counts, d_cnt.p, (size_t)S * 32, hipMemcpyDeviceToHost));
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
