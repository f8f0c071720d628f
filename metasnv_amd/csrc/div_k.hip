// metasnv_amd/csrc/div_k.hip -- metaSNV_DistDiv.py --div / --divNS on the device: compute_diversity (metaSNV_DistDiv.py:144-178)
// for every pair of samples (i <= j) of one species table, bit-exact with numpy / pandas.
//
//   single rows (keys that occur once), both values present, in the table's order:
//     nd   = np.sum(a*(1-b) + (1-a)*b)              each product rounded on its own, no FMA
//   groups (keys with m >= 2 rows): the m rows repeated m-1 times, then 1 - (pandas' Kahan groupby sum of them), per column;
//     value = np.nansum(np.outer(s1, s2)) - np.nansum(diagonal)          k = m(m-1)+1 values per column
//     gsum = np.sum(values over the groups)      (pandas' Series.sum: NaN -> 0 first)
//   result = nd without any group, gsum + nd otherwise
//
// numpy's sum of n contiguous float64 values: 0.0, plus the pairwise sum of each block of 8192 elements (the reduction's
// buffer), added one block after the other.  The pairwise sum of a block: n < 8 a plain loop from 0.0; n <= 128 eight
// accumulators r[j] over the elements j, 8 + j ... combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail; longer
// blocks split at n/2 rounded down to a multiple of 8, left + right.  np_sum below walks that tree with a small explicit
// stack and asks a leaf functor for the sum of the next `len` elements of its stream, so the elements are produced in
// order and never stored beyond the leaf that uses them.
//
// msnv_div_pairs: ONE WAVEFRONT per pair of samples.
//   single rows: the host's validity bits (one word per 64 rows per sample) give the count n up front, hence the tree;
//     the lanes then take 64 rows per step, each valid row's product lands in an LDS ring at its compacted position
//     (popcount of the lower lanes' bits), and a complete leaf is summed by eight lanes in numpy's order.
//   groups: each lane computes the value of one group (its Kahan sums, the k x k outer product and the diagonal, each a
//     numpy sum of its own with the same tree), 64 groups per step into the same ring; the G values are then summed
//     like the single rows (n = G, all present).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "msnv_internal.h"
#include "stagedev.h"

namespace msnv {

constexpr int NP_BLOCK = 8192;                               // numpy's reduction buffer
constexpr int NP_LEAF = 128;                                 // numpy's PW_BLOCKSIZE
constexpr int RING = 256;                                    // LDS ring: a leaf (<= 128) + one step of 64 fit

// numpy's pairwise sum of one block of B elements; leaf(len) returns the numpy sum of the next len elements of the stream.
// The right child is never longer than n/2 + 8, so a block of 8192 opens at most 7 frames.
template <class Leaf> __device__ double np_block(int B, Leaf &leaf) {
#pragma clang fp contract(off)
    int right[8];
    double left[8];
    int top = 0, cur = B;
    while (true) {
        while (cur > NP_LEAF) {
            int n2 = cur / 2;
            n2 -= n2 % 8;
            right[top++] = cur - n2;
            cur = n2;
        }
        double v = leaf(cur);
        while (top > 0 && right[top - 1] < 0) { --top; v = left[top] + v; }
        if (top == 0) return v;
        left[top - 1] = v;
        cur = right[top - 1];
        right[top - 1] = -1;                                  // the right child is under way
    }
}

template <class Leaf> __device__ double np_sum(long n, Leaf &leaf) {
#pragma clang fp contract(off)
    double total = 0.0;
    for (long b = 0; b < n; b += NP_BLOCK) total = total + np_block((int)min((long)NP_BLOCK, n - b), leaf);
    return total;
}

__device__ __forceinline__ double nz(double x) { return x != x ? 0.0 : x; }

// ---- per-lane streams (group values) --------------------------------------------------------------------------------------

// the k-vector of one column of one group: rows v[0..m-1] repeated m-1 times, then ref
struct GroupCol {
    const double *v;
    int m, k;
    double ref;
    __device__ double at(int t) const { return t < k - 1 ? v[t % m] : ref; }
};

// np.outer(s1, s2) in C order, NaN -> 0
struct OuterStream {
    GroupCol a, b;
    int t, u;
    double at_;
    __device__ double next() {
#pragma clang fp contract(off)
        const double x = nz(at_ * b.at(u));
        if (++u == b.k) { u = 0; ++t; if (t < a.k) at_ = a.at(t); }
        return x;
    }
};

// the diagonal s1[t] * s2[t], NaN -> 0
struct DiagStream {
    GroupCol a, b;
    int t;
    __device__ double next() {
#pragma clang fp contract(off)
        const double x = nz(a.at(t) * b.at(t));
        ++t;
        return x;
    }
};

// one lane sums `len` elements of its own stream in numpy's order
template <class Stream> struct LaneLeaf {
    Stream &s;
    __device__ double operator()(int len) {
#pragma clang fp contract(off)
        double res;
        if (len < 8) {
            res = 0.0;
            for (int k = 0; k < len; ++k) res += s.next();
            return res;
        }
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = s.next();
        const int n8 = len - len % 8;
        for (int k = 8; k < n8; k += 8)
            for (int j = 0; j < 8; ++j) r[j] += s.next();
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int k = n8; k < len; ++k) res += s.next();
        return res;
    }
};

// pandas' groupby().sum() of the m(m-1) repeated rows (group_sum: Kahan, NaN skipped, compensation reset when NaN)
__device__ double kahan_repeated(const double *v, int m) {
#pragma clang fp contract(off)
    double sum = 0.0, comp = 0.0;
    for (int rep = 0; rep < m - 1; ++rep)
        for (int t = 0; t < m; ++t) {
            const double x = v[t];
            if (x == x) {
                const double y = x - comp;
                const double s = sum + y;
                comp = s - sum - y;
                if (comp != comp) comp = 0.0;
                sum = s;
            }
        }
    return sum;
}

__device__ double group_value(const double *a, const double *b, int m) {
#pragma clang fp contract(off)
    const int k = m * (m - 1) + 1;
    const GroupCol ca{a, m, k, 1.0 - kahan_repeated(a, m)}, cb{b, m, k, 1.0 - kahan_repeated(b, m)};
    OuterStream os{ca, cb, 0, 0, ca.at(0)};
    LaneLeaf<OuterStream> lo{os};
    const double outer = np_sum((long)k * k, lo);
    DiagStream ds{ca, cb, 0};
    LaneLeaf<DiagStream> ld{ds};
    const double diag = np_sum((long)k, ld);
    return outer - diag;
}

// ---- the wavefront's stream: elements staged in the LDS ring at their compacted index ---------------------------------

// Single rows of the pair (i, j): the product of every row valid in both columns, in row order.
struct SingleFill {
    const double *x, *y;                                      // the two columns
    const unsigned long long *bx, *by;                        // their validity words (bits beyond the table are 0)
    long n_words;
    long w;                                                   // next word
    __device__ int operator()(double *ring, long filled) {   // stages the next word's products, returns how many
#pragma clang fp contract(off)
        const int lane = threadIdx.x;
        unsigned long long m = 0;
        while (m == 0 && w < n_words) { m = bx[w] & by[w]; ++w; }
        if (m == 0) return 0;
        if ((m >> lane) & 1ull) {
            const long r = (w - 1) * 64 + lane;
            const double a = x[r], b = y[r];
            const double na = 1 - a, nb = 1 - b;
            const double p1 = a * nb, p2 = na * b;
            const long idx = filled + __popcll(m & ((1ull << lane) - 1ull));
            ring[idx & (RING - 1)] = p1 + p2;
        }
        return __popcll(m);
    }
};

// Group values of the pair: lane g of the step computes group g (pandas' Series.sum skips NaN: NaN -> 0).
struct GroupFill {
    const double *x, *y;                                      // the group rows of the two columns
    const long *goff;                                         // group g = rows goff[g] .. goff[g+1]-1
    long n_groups, g;
    __device__ int operator()(double *ring, long filled) {
        const int lane = threadIdx.x;
        const long gg = g + lane;
        if (gg < n_groups) {
            const long lo = goff[gg];
            ring[(filled + lane) & (RING - 1)] = nz(group_value(x + lo, y + lo, (int)(goff[gg + 1] - lo)));
        }
        const int got = (int)min(64L, n_groups - g);
        g += 64;
        return got;
    }
};

template <class Fill> struct WaveLeaf {
    Fill &fill;
    double *ring;
    long filled, consumed;
    __device__ double operator()(int len) {
#pragma clang fp contract(off)
        while (filled < consumed + len) {
            __syncthreads();                                  // earlier reads of the slots about to be written are done
            const int got = fill(ring, filled);
            __syncthreads();
            if (got == 0) break;                              // cannot happen: n was counted from the same bits
            filled += got;
        }
        const int sub = threadIdx.x & 7;
        const long c = consumed;
        double res;
        if (len < 8) {
            res = 0.0;
            for (int k = 0; k < len; ++k) res += ring[(c + k) & (RING - 1)];
        } else {
            // every group of eight lanes replays r[0..7]; the partner's value is added in the same order in every lane
            const int n8 = len - len % 8;
            double r = ring[(c + sub) & (RING - 1)];
            for (int k = 8; k < n8; k += 8) r += ring[(c + k + sub) & (RING - 1)];
            const double a1 = r + __shfl_xor(r, 1);
            const double a2 = a1 + __shfl_xor(a1, 2);
            res = a2 + __shfl_xor(a2, 4);
            for (int k = n8; k < len; ++k) res += ring[(c + k) & (RING - 1)];
        }
        consumed += len;
        return res;
    }
};

__global__ __launch_bounds__(64) void msnv_div_pairs(const double *__restrict__ xs, const unsigned long long *__restrict__ bits, long n_single,
                                                     long n_words, const double *__restrict__ xg, const long *__restrict__ goff, long n_groups,
                                                     long n_grouped, int n_samples, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double ring[RING];
    const long pair = blockIdx.x;
    long i = 0, rem = pair;                                   // unrank (i <= j) from the row-major upper triangle
    while (rem >= n_samples - i) { rem -= n_samples - i; ++i; }
    const long j = i + rem;
    const int lane = threadIdx.x;
    const unsigned long long *bi = bits + i * n_words, *bj = bits + j * n_words;
    long n = 0;
    for (long w = lane; w < n_words; w += 64) n += __popcll(bi[w] & bj[w]);
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
    SingleFill sf{xs + i * n_single, xs + j * n_single, bi, bj, n_words, 0};
    WaveLeaf<SingleFill> ls{sf, ring, 0, 0};
    const double nd = np_sum(n, ls);
    double res = nd;
    if (n_groups > 0) {
        __syncthreads();
        GroupFill gf{xg + i * n_grouped, xg + j * n_grouped, goff, n_groups, 0};
        WaveLeaf<GroupFill> lg{gf, ring, 0, 0};
        res = np_sum(n_groups, lg) + nd;
    }
    if (lane == 0) out[i * n_samples + j] = res;
}

// One table (the rows of --div, or the N / the S rows of --divNS): xs / bits / xg sample-major as described above;
// out[i * S + j] (i <= j) receives compute_diversity(column i, column j).
int dev_div(const double *xs, const uint64_t *bits, long n_single, long n_words, const double *xg, const long *goff, long n_groups, long n_grouped,
            int n_samples, void *stream_, double *out, double *ms_kernel) {
    hipStream_t st = (hipStream_t)stream_;
    Buf d_xs, d_b, d_xg, d_go, d_out;
    const size_t S = (size_t)n_samples;
    const size_t xsb = S * (size_t)n_single * sizeof(double), bb = S * (size_t)n_words * sizeof(uint64_t);
    const size_t xgb = S * (size_t)n_grouped * sizeof(double), gob = (size_t)(n_groups + 1) * sizeof(long), ob = S * S * sizeof(double);
    MSNV_TRY(d_xs.upload(xs, xsb, st));
    MSNV_TRY(d_b.upload(bits, bb, st));
    MSNV_TRY(d_xg.upload(xg, xgb, st));
    MSNV_TRY(d_go.upload(goff, gob, st));
    MSNV_TRY(d_out.alloc(ob));
    const long n_pairs = (long)n_samples * (n_samples + 1) / 2;
    KernelTimer tm;
    MSNV_TRY(tm.begin(st));
    if (n_pairs)
        hipLaunchKernelGGL(msnv_div_pairs, dim3((unsigned)n_pairs), dim3(64), 0, st, d_xs.as<double>(), d_b.as<unsigned long long>(), n_single, n_words,
                           d_xg.as<double>(), d_go.as<long>(), n_groups, n_grouped, n_samples, d_out.as<double>());
    MSNV_TRY(tm.stop(st));
    if (ob) HIP_TRY(hipMemcpyAsync(out, d_out.p, ob, hipMemcpyDeviceToHost, st));
    MSNV_TRY(tm.wait(st));
    if (ms_kernel) *ms_kernel += tm.ms;
    return MSNV_OK;
}

}  // namespace msnv
