// metasnv_amd/csrc/hclust_k.hip -- the agglomeration behind subpopr's report heatmaps on the device (hclust of average, complete, single and
// McQuitty linkage; the rule is in include/msnv.h, the host side in hclust.cpp).
//
//   msnv_hclust_tasks_k   many (index list, method) tasks on one resident distance matrix: one workgroup per task
//
// A task is m - 1 dependent steps, so the parallelism is across tasks; inside a task the lanes share the cells of a step.  The workgroup gathers
// its task's W (full, mirrored, m x m fp64) into a scratch area of its own and keeps, per position a, in LDS:
//   dnn[a], nn[a]   the active b > a with the smallest W[a][b], the smallest b among equals, and that value (HCLUST_NONE, +inf: no such b)
//   size[a], active[a], list[]   the members of the cluster at a, whether a is still one, the rows to rescan in this step
// = 24 bytes per member (dynamic, sized by the largest task of the launch).  One step:
//   (1) the arg-min of (dnn[a], a) over the active rows, compared lexicographically, is the pair (a, b = nn[a])
//   (2) a lane per other active k: v = f(W[a][k], W[b][k]) -- rows a and b, coalesced -- to W[a][k] and its mirror W[k][a]; k < a takes (v, a) when it
//       undercuts (dnn[k], nn[k]); a k whose nn was a or b is put on the list; row a always is
//   (3) a wavefront per listed row k rescans W[k][k + 1 .. m) over the active columns
// Every cross-lane operation compares (double, index) pairs and every double is one cell's own arithmetic, so the steps are a function of the task
// alone, whatever the batch or the order in which the rows reach the list.
// Waiting: workgroup barriers only; every loop's bound is known on entry.  W is read and written by the same workgroup across barriers: no
// __restrict__ on it.  A picked row without a partner (a sum that overflowed to inf hides every candidate) ends the task with an error bit, not an index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device.h"
#include "msnv_internal.h"
#include "stagedev.h"

#pragma clang fp contract(off)

namespace msnv {

namespace {

constexpr uint32_t HC_THREADS = HCLUST_THREADS, HC_WAVE = 64, HC_WAVES = HC_THREADS / HC_WAVE;
constexpr uint32_t HCLUST_NONE = 0xffffffffu;
constexpr uint32_t HC_LDS_PER_MEMBER = 24;

struct HclustTask { unsigned long long off, w_off, step_off; uint32_t m, method; };   // its list in idx, its W in the scratch (doubles), its steps

struct Near { double v; uint32_t key; };

__device__ inline bool nearer(double v, uint32_t key, double than_v, uint32_t than_key) { return v < than_v || (v == than_v && key < than_key); }

// the smallest (value, key) over the workgroup, the same in every thread
__device__ inline Near block_nearest(Near b, double *red_v, uint32_t *red_k) {
    red_v[threadIdx.x] = b.v; red_k[threadIdx.x] = b.key;
    __syncthreads();
    for (uint32_t d = HC_THREADS / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const double ov = red_v[threadIdx.x + d];
            const uint32_t ok = red_k[threadIdx.x + d];
            if (nearer(ov, ok, red_v[threadIdx.x], red_k[threadIdx.x])) { red_v[threadIdx.x] = ov; red_k[threadIdx.x] = ok; }
        }
        __syncthreads();
    }
    Near r{red_v[0], red_k[0]};
    __syncthreads();
    return r;
}

// rows list[0 .. n_list) of W, a wavefront each: nn / dnn over the active columns behind the diagonal
__device__ inline void rescan_rows(const double *W, uint32_t m, const uint32_t *list, uint32_t n_list, const uint32_t *active, double *dnn, uint32_t *nn) {
    const uint32_t wave = threadIdx.x / HC_WAVE, lane = threadIdx.x % HC_WAVE;
    for (uint32_t r = wave; r < n_list; r += HC_WAVES) {
        const uint32_t k = list[r];
        const double *row = W + (size_t)k * m;
        double bv = INFINITY;
        uint32_t bj = HCLUST_NONE;
        for (uint32_t j = k + 1 + lane; j < m; j += HC_WAVE) {         // ascending per lane: a strict < keeps the smallest j
            if (!active[j]) continue;
            const double v = row[j];
            if (v < bv) { bv = v; bj = j; }
        }
        for (uint32_t d = HC_WAVE / 2; d > 0; d >>= 1) {
            const double ov = __shfl_xor(bv, (int)d, (int)HC_WAVE);
            const uint32_t oj = (uint32_t)__shfl_xor((int)bj, (int)d, (int)HC_WAVE);
            if (nearer(ov, oj, bv, bj)) { bv = ov; bj = oj; }
        }
        if (lane == 0) { dnn[k] = bv; nn[k] = bj; }
    }
}

}  // namespace

__global__ void __launch_bounds__(HC_THREADS) msnv_hclust_tasks_k(const double *__restrict__ D, uint32_t n, const HclustTask *__restrict__ tasks, unsigned long long n_tasks,
                                                                  const int32_t *__restrict__ idx, uint32_t lds_m, double *scratch, int32_t *__restrict__ step_a,
                                                                  int32_t *__restrict__ step_b, double *__restrict__ step_h, uint32_t *__restrict__ err) {
    extern __shared__ __align__(16) unsigned char hc_lds[];
    __shared__ double red_v[HC_THREADS];
    __shared__ uint32_t red_k[HC_THREADS];
    __shared__ uint32_t s_nlist;
    double *dnn = (double *)hc_lds;
    uint32_t *nn = (uint32_t *)(dnn + lds_m), *size = nn + lds_m, *active = size + lds_m, *list = active + lds_m;
    const uint32_t tid = threadIdx.x;
    for (unsigned long long t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const HclustTask T = tasks[t];
        const uint32_t m = T.m, method = T.method;
        double *W = scratch + T.w_off;
        __syncthreads();                                               // the task before is done with the LDS
        for (uint32_t j = tid; j < m; j += HC_THREADS) { nn[j] = (uint32_t)idx[T.off + j]; size[j] = 1; active[j] = 1; list[j] = j; }      // nn holds the columns for the gather
        __syncthreads();
        for (uint32_t r = 0; r < m; ++r) {
            const double *src = D + (size_t)nn[r] * n;
            for (uint32_t c = tid; c < m; c += HC_THREADS) W[(size_t)r * m + c] = src[nn[c]];
        }
        __syncthreads();
        rescan_rows(W, m, list, m, active, dnn, nn);                   // every row; a lane reads nn[k] of the gather no more
        __syncthreads();
        for (uint32_t s = 0; s + 1 < m; ++s) {
            // ---- (1) the pair
            Near best{INFINITY, HCLUST_NONE};
            for (uint32_t a = tid; a < m; a += HC_THREADS)
                if (active[a] && nearer(dnn[a], a, best.v, best.key)) { best.v = dnn[a]; best.key = a; }
            best = block_nearest(best, red_v, red_k);
            const uint32_t a = best.key, b = a < m ? nn[a] : HCLUST_NONE;
            if (b >= m) { if (tid == 0) atomicOr(err, 1u); break; }    // the same in every thread
            const double sa = (double)size[a], sb = (double)size[b];
            if (tid == 0) {
                step_a[T.step_off + s] = (int32_t)a; step_b[T.step_off + s] = (int32_t)b; step_h[T.step_off + s] = best.v;
                active[b] = 0; list[0] = a; s_nlist = 1;
            }
            __syncthreads();
            // ---- (2) the update of row and column a
            double *row_a = W + (size_t)a * m;
            const double *row_b = W + (size_t)b * m;
            for (uint32_t k = tid; k < m; k += HC_THREADS) {
                if (!active[k] || k == a) continue;
                const double x = row_a[k], y = row_b[k];
                double v;
                if (method == MSNV_HCLUST_AVERAGE) { const double px = sa * x, py = sb * y, sum = px + py; v = sum / (sa + sb); }
                else if (method == MSNV_HCLUST_COMPLETE) v = x > y ? x : y;
                else if (method == MSNV_HCLUST_SINGLE) v = x < y ? x : y;
                else { const double hx = 0.5 * x, hy = 0.5 * y; v = hx + hy; }
                row_a[k] = v; W[(size_t)k * m + a] = v;
                const uint32_t was = nn[k];
                if (was == a || was == b) list[atomicAdd(&s_nlist, 1u)] = k;      // at most once per k: the list holds at most m rows
                else if (k < a && nearer(v, a, dnn[k], was)) { dnn[k] = v; nn[k] = a; }
            }
            __syncthreads();
            if (tid == 0) size[a] = size[a] + size[b];
            // ---- (3) the rows whose nearest neighbour is gone or has moved
            rescan_rows(W, m, list, s_nlist, active, dnn, nn);
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side of the launch
// One launch over n_tasks tasks (include/msnv.h packs them): the caller has cut the batch so that 8 * sum(m^2) bytes of scratch are acceptable.
int dev_hclust_batch(const ClusterDev &c, uint64_t n_tasks, const uint32_t *m, const uint32_t *method, const int32_t *idx, void *stream, int32_t *step_a, int32_t *step_b,
                     double *step_h, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream;
    std::vector<HclustTask> tasks(n_tasks);
    uint64_t off = 0, w_off = 0;
    uint32_t max_m = 0;
    for (uint64_t t = 0; t < n_tasks; ++t) {
        tasks[t] = HclustTask{off, w_off, off - t, m[t], method[t]};
        off += m[t]; w_off += (uint64_t)m[t] * m[t];
        max_m = std::max(max_m, m[t]);
    }
    const uint64_t n_steps = off - n_tasks;
    Buf d_tasks, d_idx, d_w, d_a, d_b, d_h, d_err;
    MSNV_TRY(d_tasks.upload(tasks.data(), n_tasks * sizeof(HclustTask), st));
    MSNV_TRY(d_idx.upload(idx, off * 4, st));
    MSNV_TRY(d_w.alloc(w_off * 8));
    MSNV_TRY(d_a.alloc(n_steps * 4));
    MSNV_TRY(d_b.alloc(n_steps * 4));
    MSNV_TRY(d_h.alloc(n_steps * 8));
    MSNV_TRY(d_err.alloc(16));
    HIP_TRY(hipMemsetAsync(d_err.p, 0, 16, st));
    const size_t lds = (size_t)max_m * HC_LDS_PER_MEMBER;
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)msnv_hclust_tasks_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint32_t per_cu = (uint32_t)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (lds + 4096)));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tasks, dev_resident_workgroups(per_cu));
    KernelTimer tm;
    MSNV_TRY(tm.begin(st));
    hipLaunchKernelGGL(msnv_hclust_tasks_k, dim3(grid), dim3(HC_THREADS), lds, st, c.dist, c.n, d_tasks.as<HclustTask>(), (unsigned long long)n_tasks, d_idx.as<int32_t>(), max_m,
                       d_w.as<double>(), d_a.as<int32_t>(), d_b.as<int32_t>(), d_h.as<double>(), d_err.as<uint32_t>());
    MSNV_TRY(tm.stop(st));
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(step_a, d_a.p, n_steps * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(step_b, d_b.p, n_steps * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(step_h, d_h.p, n_steps * 8, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    if (ms_kernel) *ms_kernel += tm.ms;
    if (err) return fail(MSNV_EDOMAIN, "hclust: a task's distances overflowed to inf and left a cluster without a nearest neighbour");
    return MSNV_OK;
}

}  // namespace msnv
