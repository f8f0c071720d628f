// metasnv_amd/csrc/devsub.hip -- the read subsampler on the device (msnv_records_subsample_device; `qaCompute -a`, `metaSNV.py --subsample`):
// of several record streams in HBM, the records whose name hash passes the rule of devsub.h, stream by stream, contiguous and in order.
//
// The dealer's sibling (devdeal.hip) without the sort.  The streams are staged and their records found by the record scan (devscan.hip:
// stage_streams, scan_records); msnv_sub_measure (rec_load, the name's x31 hash, wang, the threshold: keep and size per record, kept /
// dropped / bytes per stream), one exclusive scan of the sizes over all records -- a stream's places are its records' sums less the sum at
// its first record --, msnv_sub_copy.  What it shares with the scan, the dealer and the round is devrec.h; the rule is devsub.h.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "devrec.h"
#include "devsub.h"

namespace msnv {

namespace {
constexpr uint32_t SUB_COPIES = 64;                    // per-stream counters in this many copies (same-address atomics: msnv_deal_measure)
struct SubAcc { unsigned long long bytes; uint32_t kept, dropped, bad, pad; };
// One thread per record: header and name from HBM (the name in 16-byte pieces: a lane's loads are its own cache lines either way, so few and
// wide), the decision, the record's size if it stays (0: it does not exist behind this stage).
__global__ __launch_bounds__(256) void msnv_sub_measure(const uint8_t *raw, const unsigned long long *rec_off, const uint16_t *rec_sample, uint32_t n_rec, const unsigned long long *s_end,
                                                        uint32_t word, uint32_t threshold, uint32_t *size, SubAcc *acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t f = 0, s = 0xffffffffu, sz = 0;            // f: 1 kept, 2 dropped, 4 malformed
    if (i < n_rec) {
        s = rec_sample[i];
        const uint8_t *p = raw + rec_off[i];
        const Rec r = rec_load(p, s_end[s] - rec_off[i]);
        if (!r.ok) f = 4u;                              // its inner fields do not fit its block_size: MSNV_EFORMAT, as in the dealer
        else {
            // the name: bytes up to the first NUL, at most l_read_name of them (r.ok: they lie inside the record; a piece's last bytes may
            // be the record's next fields, or the readable bytes behind the staged streams)
            uint32_t h = 0; bool open = true;
            for (uint32_t o = 0; o < r.l_name && open; o += 16u) {
                uint4 v; __builtin_memcpy(&v, p + 36 + o, 16);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w}, nb = r.l_name - o;
#pragma unroll
                for (uint32_t k = 0; k < 16u; ++k) {
                    const uint8_t c = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
                    open = open && k < nb && c != 0;
                    if (open) h = x31_step(h, c);
                }
            }
            if (sub_keep_hash(h, word, threshold)) { f = 1u; sz = r.bs + 4u; } else f = 2u;
        }
        size[i] = sz;
    }
    // a wavefront's records nearly always belong to one stream: ballots and one lane's atomics (msnv_deal_measure)
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    if (__all(s == s0 || f == 0u)) {
        if (s0 != 0xffffffffu) {
            const unsigned long long b0 = __ballot(f & 1u), b1 = __ballot(f & 2u), b2 = __ballot(f & 4u);
            unsigned long long sum = sz;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
            if ((threadIdx.x & 63) == 0) {
                SubAcc &a = acc[(size_t)s0 * SUB_COPIES + (blockIdx.x % SUB_COPIES)];
                if (b0) { atomicAdd(&a.kept, (uint32_t)__popcll(b0)); atomicAdd(&a.bytes, sum); }
                if (b1) atomicAdd(&a.dropped, (uint32_t)__popcll(b1));
                if (b2) a.bad = 1u;
            }
        }
    } else if (f) {
        SubAcc &a = acc[(size_t)s * SUB_COPIES + (blockIdx.x % SUB_COPIES)];
        if (f & 1u) { atomicAdd(&a.kept, 1u); atomicAdd(&a.bytes, (unsigned long long)sz); }
        if (f & 2u) atomicAdd(&a.dropped, 1u);
        if (f & 4u) a.bad = 1u;
    }
}
// sixteen lanes per kept record: 16-byte pieces of the record, any alignment on either side (msnv_deal_copy).  Record j of stream s goes to
// out_off[s] + (pos[j] - pos[first record of s]): behind the kept records of s before it.
__global__ __launch_bounds__(256) void msnv_sub_copy(const uint8_t *raw, const unsigned long long *rec_off, const uint16_t *rec_sample, const uint32_t *rec_base, const uint32_t *size,
                                                     const unsigned long long *pos, const unsigned long long *out_off, uint32_t n, uint8_t *out) {
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = (uint32_t)(gt >> 4), l = (uint32_t)gt & 15u;
    if (j >= n) return;
    const uint32_t sz = size[j];
    if (!sz) return;
    const uint32_t s = rec_sample[j];
    const uint8_t *src = raw + rec_off[j];
    uint8_t *dst = out + out_off[s] + (pos[j] - pos[rec_base[s]]);
    for (uint32_t o = 16u * l; o + 16u <= sz; o += 256u) { uint4 v; __builtin_memcpy(&v, src + o, 16); __builtin_memcpy(dst + o, &v, 16); }
    if (l == 0) for (uint32_t o = sz & ~15u; o < sz; ++o) dst[o] = src[o];
}
}  // namespace

int records_subsample_device(msnv_ctx *ctx, const uint8_t *const *streams, const uint64_t *n_bytes, int n, bool on_device, int n_contigs, uint32_t word, uint32_t threshold,
                             uint8_t *out, uint64_t capacity, uint64_t *out_off, uint64_t *out_bytes, uint64_t *counts, double *ms_kernel) {
    if (ms_kernel) *ms_kernel = 0;
    if (n <= 0) return MSNV_OK;
    if (n > 2048) return fail(MSNV_EINVAL, "msnv_records_subsample_device: at most 2048 streams per call");
    uint64_t need = 0;
    sub_layout(n_bytes, n, out_off, &need);
    if (capacity < need) return fail(MSNV_EINVAL, "msnv_records_subsample_device: the output holds %llu bytes, %llu are needed (every stream's bytes + 16, rounded up to 16)", (unsigned long long)capacity, (unsigned long long)need);
    const size_t S = (size_t)n;
    for (size_t s = 0; s < S; ++s) { out_bytes[s] = 0; counts[2 * s] = counts[2 * s + 1] = 0; }
    if (int rc = dev_set_device(ctx->device)) return rc;
    hipStream_t st = (hipStream_t)ctx->stream;
    std::vector<std::pair<void *, uint64_t>> slots;                // this call's work buffers
    struct FreeSlots { std::vector<std::pair<void *, uint64_t>> &v; ~FreeSlots() { for (auto &b : v) if (b.first) dev_free(b.first); } } free_slots{slots};
    BufPool pool{slots};
    ScanResult SR;
    if (int rc = stage_streams(st, ctx->device, pool, streams, n_bytes, S, on_device, SR)) return rc;
    if (int rc = scan_records(st, pool, n_bytes, S, (size_t)n_contigs, SR)) return rc;
    for (size_t s = 0; s < S; ++s) if (SR.bad_off[s] != ~0ull) return fail(MSNV_EFORMAT, "malformed BAM record at byte %llu of stream %zu", (unsigned long long)SR.bad_off[s], s);
    const uint32_t NR = SR.NR;
    if (ms_kernel) *ms_kernel = SR.ms_scan;
    if (!NR) return MSNV_OK;
    auto *d_size = pool.take<uint32_t>((uint64_t)NR + 1);
    auto *d_pos = pool.take<unsigned long long>((uint64_t)NR + 1);
    auto *d_outoff = pool.take<unsigned long long>(S);
    auto *d_acc = pool.take<SubAcc>(S * SUB_COPIES);
    if (pool.rc) return pool.rc;
    Prim prim(st);
    size_t tmp_need = 0;                                           // the scan's storage before anything is queued
    if (int rc = prim.exclusive(d_size, d_pos, 0ull, (size_t)NR, rocprim::plus<unsigned long long>(), &tmp_need)) return rc;
    if (int rc = prim.bind(pool, tmp_need + 16)) return rc;
    std::vector<unsigned long long> h_outoff(out_off, out_off + S);
    Timer tm(st);
    HIP_TRY(hipMemcpyAsync(d_outoff, h_outoff.data(), S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_acc, 0, S * SUB_COPIES * sizeof(SubAcc), st));
    tm.start();
    hipLaunchKernelGGL(msnv_sub_measure, grid_for(NR, 256), dim3(256), 0, st, SR.raw, SR.d_recoff, SR.d_recsample, NR, SR.d_send, word, threshold, d_size, d_acc);
    HIP_TRY(hipGetLastError());
    if (int rc = prim.exclusive(d_size, d_pos, 0ull, (size_t)NR, rocprim::plus<unsigned long long>())) return rc;
    hipLaunchKernelGGL(msnv_sub_copy, grid_for((uint64_t)NR * 16, 256), dim3(256), 0, st, SR.raw, SR.d_recoff, SR.d_recsample, SR.d_recbase, d_size, d_pos, d_outoff, NR, out);
    HIP_TRY(hipGetLastError());
    const double ms = tm.stop();
    if (ms_kernel) *ms_kernel += ms;
    std::vector<SubAcc> acc(S * SUB_COPIES);
    HIP_TRY(hipMemcpyAsync(acc.data(), d_acc, acc.size() * sizeof(SubAcc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t s = 0; s < S; ++s) {
        bool bad = false;
        for (uint32_t c = 0; c < SUB_COPIES; ++c) {
            const SubAcc &a = acc[s * SUB_COPIES + c];
            out_bytes[s] += a.bytes; counts[2 * s] += a.kept; counts[2 * s + 1] += a.dropped; bad |= a.bad != 0;
        }
        if (bad) return fail(MSNV_EFORMAT, "stream %zu: malformed BAM record (its name, CIGAR and bases do not fit its block_size)", s);
    }
    return MSNV_OK;
}

// (No warm-up kernel for msnv_ctx_create: a context that never subsamples launches nothing of this file; the first call that does loads it.)

}  // namespace msnv
