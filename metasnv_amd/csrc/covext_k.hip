// metasnv_amd/csrc/covext_k.hip -- qaCompute's -m / -p W / -x FILE outputs from the coverage index (SURVEY.md section 8 row a).
//
// msnv_coverage_extras walks the same index as msnv_coverage_tiles (cov_iv, cov_pairs, cov_work, tile_len) with the same
// difference-array rule (kernels.hip "scatter", which restates qaCompute.cpp:530-552) and feeds up to three consumers, each
// switched on only when asked for:
//   median   per (sample, contig) row a histogram WINDOW of CX_BINS 32-bit counts plus the number and the sum of the positions at a
//            negative depth (only a contig's last position can be, by the reads that hang over the end: radix.h orders it last, so
//            it is the median of a contig of one or two bases).  The first pass counts depths
//            [0, CX_FINE) one per bin and everything above in CX_BINS - CX_FINE coarse bins of 2^22 depths; a row whose rank
//            L / 2 (qaCompute.cpp:190,215) falls into a coarse bin is refined twice at most (bins of 2^11 depths, then of 1):
//            three launches whatever the depth, any depth below 2^31 comes out right.  The host picks the rank; positions of
//            tiles without a work item are depth 0 and are added there (as coverage.cpp completes bin 0).
//   profile  per row the window sums of qaCompute.cpp:173-186 as 64-bit values: index 0 and indices 1 .. W share window 0,
//            index i >= 1 lies in window (i - 1) / W.  A thread sums its positions window by window and adds with one
//            64-bit atomic per window it touches.
//   regions  per (sample, region) the sum of the depth over [start, end]; the regions of a contig come sorted by start with
//            the running maximum of their ends, so the ones that can overlap a tile are one range found by two binary searches.
//
// No per-position array exists in HBM at any time.  Extra device memory: 8 B x regions x samples + 16 B x regions +
// 16 B x rows, and per BATCH of rows (CX_ROW_WORDS x 4 B) x rows of the batch + 8 B x windows of the batch's rows; the rows are
// cut into batches of at most CX_BATCH_BYTES of those two (a single row whose windows alone exceed that runs by itself).
// A batch launches over every work item; pairs of other rows are skipped.  The kernel is not on metaSNV's path and takes the
// plain form: one workgroup per work item, the tile's depths materialised by one scan, all three consumers reading that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "msnv_internal.h"
#include "device.h"
#include "hiptry.h"

namespace msnv {

constexpr int CX_NT = 256;
constexpr int CX_PER = TILE / CX_NT;                   // consecutive positions of one thread
constexpr uint32_t CX_FINE = 1536;                     // first pass: bins of one depth ...
constexpr uint32_t CX_COARSE_SHIFT = 22;               // ... and (CX_BINS - CX_FINE) x 2^22 >= 2^31 above them
constexpr uint32_t CX_REFINE_SHIFT = 11;               // a refined window holds CX_BINS bins of 2^11, then of 1
constexpr uint32_t CX_MODE_OFF = 0xffffffffu, CX_MODE_FIRST = 0xfffffffeu;
constexpr uint64_t CX_BATCH_BYTES = 256ull << 20;
static_assert(((uint64_t)(CX_BINS - CX_FINE) << CX_COARSE_SHIFT) >= (1ull << 31), "the coarse bins reach every depth");
static_assert((uint64_t)CX_BINS << CX_REFINE_SHIFT >= (1ull << CX_COARSE_SHIFT) && CX_BINS >= (1u << CX_REFINE_SHIFT), "two refinements reach single depths");
static_assert(CX_PER * CX_NT == (int)TILE && CX_PER == 8, "a thread loads its positions as two 16-byte words");

struct CovxArgs {
    const Pair32 *iv; const TilePair *pairs; const WorkItem *work; const uint32_t *tile_len, *tile_contig, *contig_tile_base;
    uint32_t n_pairs, row_lo, row_hi;
    uint32_t *hist; const uint2 *row_param;                                     // median: [row - row_lo][CX_ROW_WORDS]; {lo, mode} per row (NULL: off)
    unsigned long long *win; const unsigned long long *row_win_off; unsigned long long win_base; uint32_t window;   // profile (window = 0: off)
    const CovxRegion *regs; const uint32_t *reg_off; unsigned long long *reg_sum; uint32_t n_regions;                // regions (0: off)
};

// exclusive prefix of x over the workgroup's threads (every thread calls it)
template <typename T>
__device__ __forceinline__ T block_exclusive(const T x, T *s_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = x;
    for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    __syncthreads();
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    T base = 0;
    for (int k = 0; k < wave; ++k) base += s_part[k];
    return base + inc - x;
}

__global__ __launch_bounds__(CX_NT) void msnv_coverage_extras(const CovxArgs a) {
    __shared__ __attribute__((aligned(16))) int s_diff[TILE];
    __shared__ long long s_pre[TILE];                        // regions: inclusive prefix sum of the depth
    __shared__ int s_part32[CX_NT / 64];
    __shared__ long long s_part64[CX_NT / 64];
    const WorkItem w = a.work[blockIdx.x];
    const uint32_t t0 = w.tile * TILE, tl = min(a.tile_len[w.tile], TILE);
    const uint32_t contig = a.tile_contig[w.tile];
    const uint32_t p0 = (w.tile - a.contig_tile_base[contig]) * TILE;       // the tile's first index inside its contig
    const uint32_t tid = threadIdx.x;
    // regions of this contig that can overlap the tile: start <= last scanned index, and some end at or before them >= p0
    uint32_t r_lo = 0, r_hi = 0;
    if (a.n_regions && tl) {
        const uint32_t lo = a.reg_off[contig], hi = a.reg_off[contig + 1], last = p0 + tl - 1u;
        uint32_t x = lo, y = hi;
        while (x < y) { const uint32_t m = x + (y - x) / 2u; if (a.regs[m].start <= last) x = m + 1u; else y = m; }
        r_hi = x;
        x = lo; y = r_hi;
        while (x < y) { const uint32_t m = x + (y - x) / 2u; if (a.regs[m].max_end < p0) x = m + 1u; else y = m; }
        r_lo = x;
    }
    for (uint32_t k = w.pair_lo; k < w.pair_hi && k < a.n_pairs; ++k) {
        const TilePair pr = a.pairs[k];
        const uint32_t row = pr.max_depth;                   // accumulator row of the pair's (sample, contig) (finalize.cpp)
        if (row < a.row_lo || row >= a.row_hi) continue;     // (the same for every thread)
        reinterpret_cast<int4 *>(s_diff)[2 * tid] = make_int4(0, 0, 0, 0);
        reinterpret_cast<int4 *>(s_diff)[2 * tid + 1] = make_int4(0, 0, 0, 0);
        __syncthreads();
        const Pair32 *v = a.iv + ((uint64_t)pr.nblk << 32 | pr.blk_lo) + pr.read_lo;
        const uint32_t n = pr.read_hi - pr.read_lo;
        for (uint32_t i = tid; i < n; i += CX_NT) {
            // kernels.hip "scatter": an interval from an earlier tile enters at 0; an end left of the tile wraps and leaves it like
            // one beyond it; {end, end - 1} has no start and its -1 at .y (qaCompute.cpp:542-549)
            const Pair32 x = v[i];
            const uint32_t m = max(x.x, t0), e = x.y - t0;
            if (x.y >= m && m - t0 < TILE) atomicAdd(&s_diff[m - t0], 1);
            if (e < TILE) atomicSub(&s_diff[e], 1);
        }
        __syncthreads();
        int dep[CX_PER];
        {
            const int4 q0 = reinterpret_cast<const int4 *>(s_diff)[2 * tid], q1 = reinterpret_cast<const int4 *>(s_diff)[2 * tid + 1];
            dep[0] = q0.x; dep[1] = q0.y; dep[2] = q0.z; dep[3] = q0.w; dep[4] = q1.x; dep[5] = q1.y; dep[6] = q1.z; dep[7] = q1.w;
        }
#pragma unroll
        for (int j = 1; j < CX_PER; ++j) dep[j] += dep[j - 1];
        const int before = block_exclusive<int>(dep[CX_PER - 1], s_part32);
#pragma unroll
        for (int j = 0; j < CX_PER; ++j) dep[j] += before;   // depth at index CX_PER * tid + j of the tile
        const uint32_t first = CX_PER * tid;
        const uint32_t mine = first < tl ? min(tl - first, (uint32_t)CX_PER) : 0u;     // scanned positions among mine (i < contig length)

        // ---- median: runs of constant depth into the row's histogram window
        const uint2 prm = a.row_param ? a.row_param[row] : make_uint2(0u, CX_MODE_OFF);
        if (prm.y != CX_MODE_OFF && mine) {
            uint32_t *h = a.hist + (uint64_t)(row - a.row_lo) * CX_ROW_WORDS;
            auto count = [&](const int d, const uint32_t len) {
                if (d < 0) { atomicAdd(&h[CX_BINS], len); atomicAdd(&h[CX_BINS + 1], (uint32_t)d * len); return; }
                uint32_t bin;
                if (prm.y == CX_MODE_FIRST) bin = (uint32_t)d < CX_FINE ? (uint32_t)d : CX_FINE + ((uint32_t)d >> CX_COARSE_SHIFT);
                else {
                    if ((uint32_t)d < prm.x) return;
                    bin = ((uint32_t)d - prm.x) >> prm.y;
                    if (bin >= CX_BINS) return;
                }
                atomicAdd(&h[bin], len);
            };
            int d = dep[0];
            uint32_t len = 0;
#pragma unroll
            for (int j = 0; j < CX_PER; ++j) {
                if ((uint32_t)j >= mine) break;
                if (dep[j] != d) { count(d, len); d = dep[j]; len = 0; }
                ++len;
            }
            count(d, len);
        }

        // ---- profile: my positions summed window by window (a run that crosses a window edge is split there)
        if (a.window && mine) {
            const unsigned long long off = a.row_win_off[row], n_win = a.row_win_off[row + 1] - off;
            unsigned long long *dst = a.win + (off - a.win_base);
            auto window_of = [&](const uint32_t p) -> uint32_t { return p ? (p - 1u) / a.window : 0u; };     // qaCompute.cpp:174-181
            uint32_t cw = window_of(p0 + first);
            unsigned long long sum = 0;
#pragma unroll
            for (int j = 0; j < CX_PER; ++j) {
                if ((uint32_t)j >= mine) break;
                const uint32_t wd = window_of(p0 + first + (uint32_t)j);
                if (wd != cw) { if (sum && cw < n_win) atomicAdd(&dst[cw], sum); cw = wd; sum = 0; }
                sum += (unsigned long long)(long long)dep[j];                      // (a -1 wraps as wSum does)
            }
            if (sum && cw < n_win) atomicAdd(&dst[cw], sum);
        }

        // ---- regions
        if (r_hi > r_lo) {
            long long pre[CX_PER];
            pre[0] = dep[0];
#pragma unroll
            for (int j = 1; j < CX_PER; ++j) pre[j] = pre[j - 1] + dep[j];
            const long long base = block_exclusive<long long>(pre[CX_PER - 1], s_part64);
#pragma unroll
            for (int j = 0; j < CX_PER; ++j) s_pre[first + j] = base + pre[j];
            __syncthreads();
            const uint32_t last = p0 + tl - 1u;
            for (uint32_t r = r_lo + tid; r < r_hi; r += CX_NT) {
                const CovxRegion g = a.regs[r];
                if (g.end < p0 || g.start > last) continue;
                const uint32_t b = max(g.start, p0) - p0, e = min(g.end, last) - p0;
                const long long s = s_pre[e] - (b ? s_pre[b - 1u] : 0ll);
                if (s) atomicAdd(&a.reg_sum[(uint64_t)pr.sample * a.n_regions + g.id], (unsigned long long)s);
            }
        }
        __syncthreads();                                     // s_diff and s_pre are free for the next pair
    }
}

// ------------------------------------------------------------------------------------------ host side
namespace {
struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() { for (void *q : p) dev_free(q); }
    template <typename T> int get(T **out, uint64_t n) {
        void *q = nullptr;
        if (int rc = dev_alloc(&q, std::max<uint64_t>(1, n) * sizeof(T), nullptr)) return rc;
        p.push_back(q);
        *out = (T *)q;
        return MSNV_OK;
    }
};
}  // namespace

int dev_run_coverage_extras(DeviceCols &d, CovxJob &job, void *stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const uint64_t n_rows = d.n_cov_rows;
    const uint32_t n_reg = (uint32_t)job.regs.size();
    job.row_median.assign((size_t)n_rows, 0);
    job.win.assign(job.window ? (size_t)job.row_win_off[(size_t)n_rows] : 0, 0);
    job.reg_sum.assign((size_t)job.n_samples * n_reg, 0);
    job.n_launches = 0;
    if (!n_rows || !d.n_cov_work || (!job.want_median && !job.window && !n_reg)) return MSNV_OK;
    if (job.row_contig.size() != n_rows || job.row_len.size() != n_rows || job.row_scanned.size() != n_rows || job.row_win_off.size() != n_rows + 1 ||
        job.contig_tile_base.size() != d.n_contigs || job.reg_off.size() != (size_t)d.n_contigs + 1)
        return fail(MSNV_EINVAL, "coverage extras: the job's tables do not match the dataset");

    DevBufs bufs;
    CovxArgs a{};
    a.iv = d.cov_iv; a.pairs = d.cov_pairs; a.work = d.cov_work; a.tile_len = d.tile_len; a.tile_contig = d.tile_contig_dev; a.n_pairs = d.n_cov_pairs;
    uint32_t *ctb = nullptr;
    if (int rc = bufs.get(&ctb, d.n_contigs)) return rc;
    if (int rc = dev_upload(ctb, job.contig_tile_base.data(), (uint64_t)d.n_contigs * 4)) return rc;
    a.contig_tile_base = ctb;
    uint2 *param = nullptr;
    std::vector<uint2> h_param;
    if (job.want_median) {
        if (int rc = bufs.get(&param, n_rows)) return rc;
        h_param.assign((size_t)n_rows, make_uint2(0u, CX_MODE_FIRST));
    }
    unsigned long long *win_off = nullptr;
    if (job.window) {
        if (int rc = bufs.get(&win_off, n_rows + 1)) return rc;
        if (int rc = dev_upload(win_off, job.row_win_off.data(), (n_rows + 1) * 8)) return rc;
    }
    CovxRegion *regs = nullptr; uint32_t *reg_off = nullptr; unsigned long long *reg_sum = nullptr;
    if (n_reg) {
        if (int rc = bufs.get(&regs, n_reg)) return rc;
        if (int rc = bufs.get(&reg_off, (uint64_t)d.n_contigs + 1)) return rc;
        if (int rc = bufs.get(&reg_sum, job.reg_sum.size())) return rc;
        if (int rc = dev_upload(regs, job.regs.data(), (uint64_t)n_reg * sizeof(CovxRegion))) return rc;
        if (int rc = dev_upload(reg_off, job.reg_off.data(), ((uint64_t)d.n_contigs + 1) * 4)) return rc;
        HIP_TRY(hipMemsetAsync(reg_sum, 0, job.reg_sum.size() * 8, st));
    }

    // batches of rows: histogram windows + window sums of a batch stay below CX_BATCH_BYTES
    const uint64_t hist_row_bytes = job.want_median ? (uint64_t)CX_ROW_WORDS * 4 : 0;
    auto win_count = [&](uint64_t lo, uint64_t hi) -> uint64_t { return job.window ? job.row_win_off[(size_t)hi] - job.row_win_off[(size_t)lo] : 0; };
    std::vector<uint32_t> h_hist;
    for (uint64_t lo = 0; lo < n_rows;) {
        uint64_t hi = lo + 1;
        while (hi < n_rows && (hi + 1 - lo) * hist_row_bytes + win_count(lo, hi + 1) * 8 <= CX_BATCH_BYTES) ++hi;
        const uint64_t nb = hi - lo, n_win = win_count(lo, hi);
        DevBufs batch;
        uint32_t *hist = nullptr; unsigned long long *win = nullptr;
        if (job.want_median) if (int rc = batch.get(&hist, nb * CX_ROW_WORDS)) return rc;
        if (n_win) if (int rc = batch.get(&win, n_win)) return rc;
        std::vector<uint64_t> rem(job.want_median ? (size_t)nb : 0);          // rank still to go inside the row's window
        for (uint64_t r = 0; r < (uint64_t)rem.size(); ++r) rem[(size_t)r] = job.row_len[(size_t)(lo + r)] / 2;
        for (int pass = 0; pass < 3; ++pass) {
            a.row_lo = (uint32_t)lo; a.row_hi = (uint32_t)hi;
            a.hist = hist; a.row_param = param;
            const bool first = pass == 0;
            a.win = first ? win : nullptr; a.row_win_off = win_off; a.win_base = job.window ? job.row_win_off[(size_t)lo] : 0; a.window = first && n_win ? job.window : 0u;
            a.regs = regs; a.reg_off = reg_off; a.reg_sum = reg_sum; a.n_regions = first ? n_reg : 0u;
            if (job.want_median) {
                HIP_TRY(hipMemcpyAsync(param + lo, h_param.data() + lo, nb * sizeof(uint2), hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemsetAsync(hist, 0, nb * CX_ROW_WORDS * 4, st));
            }
            if (a.window) HIP_TRY(hipMemsetAsync(win, 0, n_win * 8, st));
            hipLaunchKernelGGL(msnv_coverage_extras, dim3(d.n_cov_work), dim3(CX_NT), 0, st, a);
            HIP_TRY(hipGetLastError());
            ++job.n_launches;
            if (a.window) HIP_TRY(hipMemcpyAsync(job.win.data() + job.row_win_off[(size_t)lo], win, n_win * 8, hipMemcpyDeviceToHost, st));
            if (job.want_median) {
                h_hist.resize((size_t)(nb * CX_ROW_WORDS));
                HIP_TRY(hipMemcpyAsync(h_hist.data(), hist, nb * CX_ROW_WORDS * 4, hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(hipStreamSynchronize(st));
            if (!job.want_median) break;
            // the element of rank L / 2 in unsigned order (qaCompute.cpp:190,215): depths ascending, the negative ones last
            bool again = false;
            for (uint64_t r = 0; r < nb; ++r) {
                uint2 &pm = h_param[(size_t)(lo + r)];
                if (pm.y == CX_MODE_OFF) continue;
                const uint32_t *h = h_hist.data() + (size_t)(r * CX_ROW_WORDS);
                const uint64_t L = job.row_len[(size_t)(lo + r)];
                uint64_t cum = 0;
                uint32_t bin = CX_BINS;
                for (uint32_t b = 0; b < CX_BINS; ++b) {
                    uint64_t c = h[b];
                    // tiles without a work item: depth 0 throughout (coverage.cpp completes bin 0 the same way)
                    if (first && b == 0 && L > job.row_scanned[(size_t)(lo + r)]) c += L - job.row_scanned[(size_t)(lo + r)];
                    if (rem[(size_t)r] < cum + c) { bin = b; break; }
                    cum += c;
                }
                if (bin == CX_BINS) {
                    if (!first || cum + h[CX_BINS] != L)
                        return fail(MSNV_EHIP, "coverage extras: the depth histogram of row %llu does not add up to its contig (pass %d)", (unsigned long long)(lo + r), pass);
                    // the rank lies among the negative depths, which order last: one position at most, whose depth is their sum
                    if (h[CX_BINS] != 1) return fail(MSNV_EHIP, "coverage extras: row %llu holds %u positions at a negative depth", (unsigned long long)(lo + r), h[CX_BINS]);
                    job.row_median[(size_t)(lo + r)] = (int32_t)h[CX_BINS + 1];
                    pm.y = CX_MODE_OFF;
                    continue;
                }
                rem[(size_t)r] -= cum;
                if (first && bin < CX_FINE) { job.row_median[(size_t)(lo + r)] = (int32_t)bin; pm.y = CX_MODE_OFF; }
                else if (first) { pm.x = std::max<uint32_t>(CX_FINE, (bin - CX_FINE) << CX_COARSE_SHIFT); pm.y = CX_REFINE_SHIFT; again = true; }
                else if (pm.y == 0) { job.row_median[(size_t)(lo + r)] = (int32_t)(pm.x + bin); pm.y = CX_MODE_OFF; }
                else { pm.x += bin << pm.y; pm.y = 0; again = true; }
            }
            if (!again) break;
        }
        lo = hi;
    }
    if (n_reg) {
        HIP_TRY(hipMemcpyAsync(job.reg_sum.data(), reg_sum, job.reg_sum.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MSNV_OK;
}

}  // namespace msnv
