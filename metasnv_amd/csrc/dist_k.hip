// metasnv_amd/csrc/dist_k.hip -- metaSNV_DistDiv.py --dist on the device.
//
//   computeDist   metaSNV_DistDiv.py:105-124: for every pair of samples of one species' *.filtered.freq table
//     mann   = np.abs(d1 - d2).mean()            pandas: NaN (= "-1" in the file) skipped, sum / count of the rest
//     allele = (np.abs(d1 - d2) > 0.6).mean()    NaN compares False and still counts in the denominator
//
// Bit-exact floating point: pandas' nanmean is `values.sum() / count` on the float64 array with NaN replaced by 0,
// and numpy's sum of a contiguous float64 array is 0.0 plus the PAIRWISE sum of each 8192-element block (the reduction's
// buffer size), added one block after the other.  The pairwise sum of one block: pieces of <= 128 elements accumulated in 8
// interleaved partial sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail; longer pieces split at
// n/2 rounded down to a multiple of 8, recursively.  One wavefront per sample pair replays exactly that order for any
// table length (div_k.hip's np_sum is the same rule, one thread per sum), so the printed repr() of every distance
// equals the reference's.  No multiplications: nothing for the compiler to contract.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "msnv_internal.h"
#include "stagedev.h"

namespace msnv {

__device__ __forceinline__ double absdiff0(const double *__restrict__ x, const double *__restrict__ y, long k) {
    const double a = x[k], b = y[k];
    return (a != a || b != b) ? 0.0 : fabs(a - b);            // NaN -> 0 (pandas nanops: fill_value 0)
}

// numpy's summation as data: the leaves (pieces of <= 128 elements, in array order, none crossing an 8192-element block) and
// the order in which their sums are combined (a postfix program run on a stack that starts as [0.0]: 0 = take the next leaf,
// 1 = add the two on top; every block ends with the 1 that folds it into the running total) -- the same for every pair of
// samples, built once on the host from n_pos.  The stack never holds more than 1 + 8 values (a block splits 7 times at most;
// s_stack has 64).  ONE WAVEFRONT per pair of samples: eight lanes share a leaf, lane j accumulating the elements
// j, 8 + j, 16 + j ... exactly like numpy's r[j], so every load instruction of the wavefront reads whole 64-byte lines
// (the first form had one thread per pair walking two rows: lane stride n_pos x 8 bytes, nothing coalesced, device recursion).
struct DistLeaf { long lo; int n; int pad; };
// Leaf sums are kept in LDS up to 2048 leaves, beyond that in global scratch ([pair][leaf]).  A full block is exactly 64 leaves
// and a partial one at most 65, so the shortest table in scratch has 31 full blocks and a last block of 65 leaves: n_pos =
// 31 * 8192 + 7689 = 261641.  From there to 32 whole blocks (n_pos = 262144, LDS) the route alternates with the last block's
// 64 or 65 leaves, and everything longer is in scratch: the route follows the leaf count, not the length.
constexpr long DIST_BLOCK = 8192;                             // numpy's reduction buffer, in elements
constexpr int DIST_MAX_LEAVES_LDS = 2048;

__global__ __launch_bounds__(64) void msnv_dist_pairs(const double *__restrict__ xt, int n_samples, long n_pos, double threshold,
                                                      const DistLeaf *__restrict__ leaves, int n_leaves, const unsigned char *__restrict__ prog, int n_prog,
                                                      double *__restrict__ scratch, double *__restrict__ mann, double *__restrict__ allele) {
    __shared__ double s_leaf[DIST_MAX_LEAVES_LDS];
    __shared__ double s_stack[64];
    const long pair = blockIdx.x;
    // unrank (i <= j) from the row-major upper triangle
    long i = 0, rem = pair;
    while (rem >= n_samples - i) { rem -= n_samples - i; ++i; }
    const long j = i + rem;
    const double *x = xt + i * n_pos, *y = xt + j * n_pos;
    const int lane = threadIdx.x, sub = lane & 7, grp = lane >> 3;
    double *leaf_sum = n_leaves <= DIST_MAX_LEAVES_LDS ? s_leaf : scratch + (long)pair * n_leaves;
    long count = 0, above = 0;
    for (int l = grp; l < n_leaves; l += 8) {
        const DistLeaf lf = leaves[l];
        double res;
        if (lf.n < 8) {                                          // a table or a last block shorter than 8 positions: plain left-to-right sum
            res = 0.0;
            for (int k = 0; k < lf.n; ++k) res += absdiff0(x, y, lf.lo + k);
        } else {
            const int n8 = lf.n - (lf.n % 8);
            double r = absdiff0(x, y, lf.lo + sub);              // r[sub]
            for (int k = 8; k < n8; k += 8) r += absdiff0(x, y, lf.lo + k + sub);
            // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)): the partner's value is added in the same order in every lane
            const double a1 = r + __shfl_xor(r, 1);              // lanes 0,1 hold r0 + r1 (lane 1 computes r1 + r0: the same double)
            const double a2 = a1 + __shfl_xor(a1, 2);
            res = a2 + __shfl_xor(a2, 4);
            for (int k = n8; k < lf.n; ++k) res += absdiff0(x, y, lf.lo + k);
        }
        if (sub == 0) leaf_sum[l] = res;
        // counts (order does not matter): every lane looks at its own elements
        for (int k = sub; k < lf.n; k += 8) {
            const double a = x[lf.lo + k], b = y[lf.lo + k];
            const bool ok = !(a != a || b != b);
            count += ok ? 1 : 0;
            above += (ok && fabs(a - b) > threshold) ? 1 : 0;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) { count += __shfl_xor(count, o); above += __shfl_xor(above, o); }
    __syncthreads();
    if (lane == 0) {
        int sp = 1, next = 0;
        s_stack[0] = 0.0;                                        // the running total numpy's reduction starts from
        for (int k = 0; k < n_prog; ++k) {
            if (prog[k] == 0) s_stack[sp++] = leaf_sum[next++];
            else { --sp; s_stack[sp - 1] = s_stack[sp - 1] + s_stack[sp]; }
        }
        const double sum = s_stack[0];
        const double nanv = nan("");
        const double m = count > 0 ? sum / (double)count : nanv;
        const double al = n_pos > 0 ? (double)above / (double)n_pos : nanv;
        mann[i * n_samples + j] = m; mann[j * n_samples + i] = m;
        allele[i * n_samples + j] = al; allele[j * n_samples + i] = al;
    }
}

// the leaves and the combination order of numpy's pairwise sum over n elements (numpy/core/src/umath/loops_utils.h pairwise_sum)
static void pairwise_plan(long lo, long n, std::vector<DistLeaf> &leaves, std::vector<unsigned char> &prog) {
    if (n <= 128) { leaves.push_back(DistLeaf{lo, (int)n, 0}); prog.push_back(0); return; }
    long n2 = n / 2;
    n2 -= n2 % 8;
    pairwise_plan(lo, n2, leaves, prog);
    pairwise_plan(lo + n2, n - n2, leaves, prog);
    prog.push_back(1);
}

int dev_dist(const double *xt_host, int n_samples, long n_pos, double threshold, void *stream_, double *mann, double *allele, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    Buf d_x, d_m, d_a;
    const size_t xb = (size_t)n_samples * (size_t)n_pos * sizeof(double), mb = (size_t)n_samples * n_samples * sizeof(double);
    MSNV_TRY(d_x.upload(xt_host, xb, st));
    MSNV_TRY(d_m.alloc(mb));
    MSNV_TRY(d_a.alloc(mb));
    std::vector<DistLeaf> leaves; std::vector<unsigned char> prog;
    for (long lo = 0; lo < n_pos; lo += DIST_BLOCK) {           // 0.0 + pw(block 0) + pw(block 1) + ...
        pairwise_plan(lo, std::min(DIST_BLOCK, n_pos - lo), leaves, prog);
        prog.push_back(1);
    }
    const long n_pairs = (long)n_samples * (n_samples + 1) / 2;
    Buf d_l, d_p, d_s;
    MSNV_TRY(d_l.upload(leaves.data(), leaves.size() * sizeof(DistLeaf), st));
    MSNV_TRY(d_p.upload(prog.data(), prog.size(), st));
    if ((int)leaves.size() > DIST_MAX_LEAVES_LDS) MSNV_TRY(d_s.alloc((size_t)n_pairs * leaves.size() * sizeof(double)));
    KernelTimer tm;
    MSNV_TRY(tm.begin(st));
    if (n_pairs)
        hipLaunchKernelGGL(msnv_dist_pairs, dim3((unsigned)n_pairs), dim3(64), 0, st, d_x.as<double>(), n_samples, n_pos, threshold, d_l.as<DistLeaf>(),
                           (int)leaves.size(), d_p.as<unsigned char>(), (int)prog.size(), d_s.as<double>(), d_m.as<double>(), d_a.as<double>());
    MSNV_TRY(tm.stop(st));
    if (mb) HIP_TRY(hipMemcpyAsync(mann, d_m.p, mb, hipMemcpyDeviceToHost, st));
    if (mb) HIP_TRY(hipMemcpyAsync(allele, d_a.p, mb, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
