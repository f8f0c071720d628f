// metasnv_amd/csrc/devscan.hip -- the record scan: where the BAM records of staged streams begin.  What a round of the per-read stage
// (devpack.hip: the careful route) and the device dealer (devdeal.hip) start from; the round's quick front shares the sub-segment walk.
//
// What it replaces: sam_read1 one record at a time (qaCompute.cpp:441) -- the records are a chain, each says where the
// next one starts.
//   stage_streams         the streams side by side in one device buffer (or where they lie: in place); nothing is scanned
//   scan_records          scan_sub_walk, and scan_segments for what it leaves (and under MSNV_SCAN=segments)
//   scan_sub_walk         the quick way: msnv_scan_sub, one LANE per sub-segment of a few kilobytes (scan_sub_body over WalkPlain: a guessed entry, the
//                         records' offsets into slots); the seams checked and repaired on the device (SubWalk::settle: msnv_scan_check,
//                         msnv_scan_fix); one scan of the counts; msnv_scan_write, the offsets in record order
//   scan_segments         the careful way: msnv_scan_segments, a wavefront per segment of MSNV_SCAN_SEG_KB through LDS windows, seams checked on the
//                         host, msnv_compact_offsets; words malformed input
//   SubWalk               the bodies of its out-of-line members: the walk's buffers, and the two steps of the seam loop that are this file's kernels
// The device side of the walk that the routes share -- Rec, sub_of, guess_entry, scan_sub_body, scan_fix_body, wave_records -- is devrec.h.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "devrec.h"

namespace msnv {

namespace {

// ------------------------------------------------------------------------------------------ record boundaries
// The records of a BAM are a chain: the next one starts block_size + 4 bytes behind this one (qaCompute.cpp:441 reads them with sam_read1
// one at a time).  A stream is cut into segments of MSNV_SCAN_SEG_KB (256 KB); one wavefront per segment stages 16 KB windows of it in LDS
// (sixteen 16-byte loads per lane in flight, the next window fetched while this one is walked) and walks the chain there.  Where does the
// chain enter a segment that is not a stream's first?  The wavefront looks for the first offset whose 36 header bytes are those of a
// plausible record (sizes consistent, contig ids in range) and whose two successors are too -- a GUESS, 64 offsets tested per step --
// and the host then checks every seam: a segment's walk must end exactly where the next segment's began.  Accepted seams make the
// concatenated chain the true one by induction from offset 0; a segment that guessed wrong is walked again from the true entry point
// (never seen on real streams; tests force it).
constexpr uint32_t SCAN_WIN = 16384;
struct ScanSeg { unsigned long long beg, end, s_end, start, out_base; };     // [beg, end) of the round buffer, the stream's end, forced entry point or ~0 (search), first slot of tmp_off
struct ScanOut { unsigned long long first, stop, bad; uint32_t cnt, pad; };  // entry point used (~0: none found), where the walk stopped (first record start >= end), malformed chain at (~0: none)

__device__ __forceinline__ uint32_t lds_u32(const uint32_t *w32, uint32_t o) { return __builtin_amdgcn_alignbyte(w32[(o >> 2) + 1], w32[o >> 2], o & 3u); }
// plausibility of a record header at absolute offset o (fields from global memory, unaligned)
__device__ __forceinline__ bool plausible_at(const uint8_t *raw, unsigned long long o, unsigned long long s_end, int n_contigs, uint32_t &bs_out) {
    if (s_end - o < 36) return false;
    const Rec r = rec_load(raw + o, s_end - o);
    bs_out = r.bs;
    return r.ok && r.tid >= -1 && r.tid < n_contigs && r.pos >= -1 && r.l_name >= 1 && r.mtid >= -1 && r.mtid < n_contigs && r.mpos >= -1 && r.bs < (1u << 28);
}

__global__ __launch_bounds__(64) void msnv_scan_segments(const uint8_t *raw, const ScanSeg *segs, uint32_t n_segs, int n_contigs, unsigned long long *tmp_off, ScanOut *outs) {
    __shared__ uint4 win[SCAN_WIN / 16 + 1];
    __shared__ unsigned long long obuf[64];
    const uint32_t sg = blockIdx.x, lane = threadIdx.x;
    if (sg >= n_segs) return;
    const ScanSeg S = segs[sg];
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(win);
    unsigned long long wlo = 0, whi = 0;                         // window = [wlo, whi) of the round buffer, wlo on 16 bytes
    unsigned long long plo = ~0ull, phi = 0;                     // the prefetched window (in registers)
    uint4 pre[16];
    auto fetch = [&](unsigned long long lo, unsigned long long &hi_out) {   // 16 KB from lo (on 16 bytes) into registers, clipped to the stream (+ 16 bytes: the round buffer has slack)
        const unsigned long long lim = (S.s_end + 15) & ~15ull;
        const unsigned long long hi = lo + SCAN_WIN < lim ? lo + SCAN_WIN : lim;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned long long a = lo + 16ull * (64u * k + lane);
            pre[k] = a < hi ? *reinterpret_cast<const uint4 *>(raw + a) : make_uint4(0, 0, 0, 0);
        }
        hi_out = hi;
    };
    auto commit = [&]() {                                        // registers -> LDS
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) win[64 * k + lane] = pre[k];
        __syncthreads();
    };
    auto need = [&](unsigned long long from, unsigned long long upto) {     // make [from, upto) readable from LDS (upto - from <= a few hundred bytes)
        if (from >= wlo && upto <= whi) return;
        const unsigned long long lo = from & ~15ull;
        if (!(plo != ~0ull && lo >= plo && upto <= phi)) { plo = lo; fetch(plo, phi); }
        commit();
        wlo = plo; whi = phi;
        plo = whi >= 16 ? whi - 16 : 0;                          // the chain enters the next window within its first 16 bytes, unless a record jumps over it
        if (plo < ((S.s_end + 15) & ~15ull)) fetch(plo, phi); else plo = ~0ull;
    };
    // ---- entry point
    unsigned long long first = S.start;
    if (first == ~0ull) {
        for (unsigned long long base = S.beg; base < S.end && first == ~0ull; base += 64) {
            const unsigned long long o = base + lane;
            const unsigned long long upto = base + 64 + 36 < S.s_end ? base + 64 + 36 : S.s_end;
            need(base, upto);
            bool ok = o < S.end && S.s_end - o >= 36;
            uint32_t bs = 0;
            if (ok) {
                const uint32_t b = (uint32_t)(o - wlo);
                bs = lds_u32(w32, b);
                const int32_t tid = (int32_t)lds_u32(w32, b + 4), pos = (int32_t)lds_u32(w32, b + 8);
                const uint32_t w = lds_u32(w32, b + 12), fn = lds_u32(w32, b + 16);
                const int32_t l_seq = (int32_t)lds_u32(w32, b + 20), mtid = (int32_t)lds_u32(w32, b + 24), mpos = (int32_t)lds_u32(w32, b + 28);
                const uint32_t l_name = w & 0xffu, n_cigar = fn & 0xffffu;
                const unsigned long long needb = 36ull + l_name + 4ull * n_cigar + ((unsigned long long)(uint32_t)l_seq + 1) / 2 + (unsigned long long)(uint32_t)l_seq;
                ok = (int32_t)bs >= 32 && bs < (1u << 28) && (unsigned long long)bs + 4 <= S.s_end - o && tid >= -1 && tid < n_contigs && pos >= -1 && l_name >= 1 &&
                     l_seq >= 0 && needb <= (unsigned long long)bs + 4 && mtid >= -1 && mtid < n_contigs && mpos >= -1;
            }
            if (ok) {                                            // its two successors (global memory: few lanes get here)
                unsigned long long o2 = o + 4ull + bs;
                for (int d = 0; d < 2 && ok && o2 < S.s_end; ++d) { uint32_t b2 = 0; ok = plausible_at(raw, o2, S.s_end, n_contigs, b2); o2 += 4ull + b2; }
            }
            const unsigned long long m = __ballot(ok);
            if (m) first = base + (unsigned long long)__builtin_ctzll(m);
        }
    }
    // ---- walk
    unsigned long long off = first, bad = ~0ull, stop = ~0ull;
    unsigned long long *out = tmp_off + S.out_base;
    uint32_t cnt = 0;
    if (first != ~0ull) {
        while (off < S.end) {
            if (S.s_end - off < 36) { bad = off; break; }
            need(off, off + 4);
            const uint32_t bs = lds_u32(w32, (uint32_t)(off - wlo));
            if ((int32_t)bs < 32 || (unsigned long long)bs + 4 > S.s_end - off) { bad = off; break; }
            if (lane == 0) obuf[cnt & 63u] = off;
            ++cnt;
            if ((cnt & 63u) == 0u) { __syncthreads(); out[cnt - 64u + lane] = obuf[lane]; __syncthreads(); }
            off += 4ull + bs;
        }
        stop = off;
        __syncthreads();
        if (lane < (cnt & 63u)) out[(cnt & ~63u) + lane] = obuf[lane];
    }
    if (lane == 0) outs[sg] = ScanOut{first, stop, bad, cnt, 0u};
}

// The plain Walk (devrec.h: what scan_sub_body and scan_fix_body ask of one): the records' offsets and nothing else.
struct WalkPlain {
    struct Sums {};
    const uint8_t *raw; uint16_t *delta;
    static __device__ __forceinline__ Sums none() { return Sums{}; }
    __device__ __forceinline__ bool walk(uint32_t g, unsigned long long entry, unsigned long long b, unsigned long long e, unsigned long long s_end, uint32_t cap, Sums &,
                                         uint32_t &n, unsigned long long &off) const {
        uint16_t *dl = delta + (size_t)g * cap;
        n = 0; off = entry;
        while (off < e) {
            if (s_end - off < 36) return false;
            const uint32_t bs = ld32(raw + off);
            if ((int32_t)bs < 32 || (unsigned long long)bs + 4 > s_end - off) return false;
            if (n < cap) dl[n] = (uint16_t)(off - b);
            ++n;
            off += 4ull + bs;
        }
        return true;
    }
    __device__ __forceinline__ void keep(uint32_t, const Sums &) const {}
};
__global__ __launch_bounds__(256) void msnv_scan_sub(const uint8_t *raw, const SubStream *ss, uint32_t n_streams, uint32_t n_sub, uint32_t sub_bytes, uint32_t cap, int n_contigs,
                                                     unsigned long long *first, unsigned long long *stop, uint32_t *cnt, uint16_t *delta, uint32_t *flags) {
    scan_sub_body(raw, ss, n_streams, n_sub, sub_bytes, cap, n_contigs, first, stop, cnt, flags, WalkPlain{raw, delta});
}
// Seams of the quick scan, checked AND repaired (round 5): a sub-segment whose walk did not begin where the chain of the earlier ones stands
// (stop_max: running maximum of their ends) guessed wrong -- a false header inside a read name or a quality string: one in ~1e7 sub-segments,
// i.e. several in every round of BASELINE configs[2], where sending the whole round through the careful kernel cost 3 x the scan (85 of 128 ms).
// Only the FIRST such sub-segment of a stream can be trusted to be wrong (everything in front of it is the true chain; a wrong walk's end --
// it may lie a whole stream further on -- makes the ones behind it LOOK wrong): msnv_scan_check finds it, msnv_scan_fix walks it again from the
// true entry, the host scans the ends again and asks once more -- as many passes as the worst stream has wrong guesses (usually none).
// Flags: 2 = a sub-segment was fixed, 4 = the chain breaks from its TRUE entry (malformed input: the careful kernel words the error).
__global__ void msnv_scan_check(const SubStream *ss, uint32_t n_streams, uint32_t n_sub, uint32_t sub_bytes, const unsigned long long *first, const unsigned long long *stop_max, uint32_t *cnt, uint32_t *first_bad) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_sub) { if (g == n_sub) cnt[g] = 0; return; }
    const Sub u = sub_of(ss, n_streams, g, sub_bytes);
    if (g == u.S.sub0) return;                                      // (entered at the stream's first byte)
    const unsigned long long cur = chain_before(u, stop_max, g);
    const unsigned long long want = cur >= u.e ? ~0ull : cur;       // cur >= e: a record runs across the whole sub-segment, nothing starts here
    if (first[g] != want) atomicMin(&first_bad[u.si], g);
}
__global__ void msnv_scan_fix(const uint8_t *raw, const SubStream *ss, uint32_t n_streams, uint32_t sub_bytes, uint32_t cap, unsigned long long *first, unsigned long long *stop,
                              const unsigned long long *stop_max, uint32_t *cnt, uint16_t *delta, uint32_t *first_bad, uint32_t *flags) {
    scan_fix_body(ss, n_streams, sub_bytes, cap, first, stop, stop_max, cnt, first_bad, flags, WalkPlain{raw, delta});
}
struct U64Max { __device__ __host__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; } };
// the offsets out
__global__ __launch_bounds__(256) void msnv_scan_write(const SubStream *ss, uint32_t n_streams, uint32_t n_sub, uint32_t sub_bytes, uint32_t cap, const uint32_t *cnt, const uint32_t *base,
                                                       const uint16_t *delta, unsigned long long *rec_off, uint16_t *rec_sample, uint32_t *rec_base) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u, g0 = g - lane;
    if (g0 >= n_sub) return;
    uint32_t si = 0, w = 0xffffffffu; unsigned long long b = 0;
    if (g < n_sub) {
        const Sub u = sub_of(ss, n_streams, g, sub_bytes);
        si = u.si; b = u.b;
        w = base[g];
        if (g == u.S.sub0) rec_base[si] = w;
    }
    const uint32_t n_here = (n_sub - g0 < 64u ? n_sub - g0 : 64u);
    const uint32_t j_hi = base[g0 + n_here];                        // (base has n_sub + 1 entries)
    wave_records(w, n_here, j_hi, [&](uint32_t j, uint32_t lo) {
        const uint32_t wt = __shfl(w, (int)lo), st = __shfl(si, (int)lo);
        const unsigned long long bt = __shfl(b, (int)lo);
        if (j < j_hi) { rec_off[j] = bt + delta[(size_t)(g0 + lo) * cap + (j - wt)]; rec_sample[j] = (uint16_t)st; }
    });
}

struct CompactSeg { unsigned long long src; uint32_t dst, cnt, sample, pad; };
__global__ void msnv_compact_offsets(const unsigned long long *tmp_off, const CompactSeg *segs, unsigned long long *rec_off, uint16_t *rec_sample) {
    const CompactSeg c = segs[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < c.cnt; k += blockDim.x) { rec_off[c.dst + k] = tmp_off[c.src + k]; rec_sample[c.dst + k] = (uint16_t)c.sample; }
}

}  // namespace

// The round's streams side by side in one buffer: every stream starts on 16 bytes, readable bytes behind the last.  Nothing is scanned.
int stage_streams(hipStream_t st, const int device, BufPool &pool, const uint8_t *const *streams, const uint64_t *n_bytes, const size_t S, const bool on_device, ScanResult &R,
                  const uint8_t *in_place_base) {
    R.s_beg.assign(S, 0); R.s_end.assign(S, 0);
    if (in_place_base) {
        // the streams where they lie: offsets into the caller's buffer (api.cpp / bamfeed.cpp have checked order, alignment of the base and the bytes behind the last)
        for (size_t s = 0; s < S; ++s) { R.s_beg[s] = (unsigned long long)(streams[s] - in_place_base); R.s_end[s] = R.s_beg[s] + n_bytes[s]; }
        R.raw = const_cast<uint8_t *>(in_place_base);
        for (size_t s = 0; s < S; ++s) R.raw_bytes += n_bytes[s];     // (accounting: the records' bytes)
        return MSNV_OK;
    }
    for (size_t s = 0; s < S; ++s) { R.s_beg[s] = R.raw_bytes; R.s_end[s] = R.raw_bytes + n_bytes[s]; R.raw_bytes += (n_bytes[s] + 15 + 16) & ~15ull; }
    uint8_t *const raw = pool.take<uint8_t>(R.raw_bytes + 256);
    if (pool.rc) return pool.rc;
    const double t0 = now_s();
    if (on_device) {
        for (size_t s = 0; s < S; ++s) if (n_bytes[s]) HIP_TRY(hipMemcpyAsync(raw + R.s_beg[s], streams[s], n_bytes[s], hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        // pageable host memory: a few copies in flight keep the link busy (the runtime stages them)
        std::atomic<size_t> next{0}; std::atomic<int> bad{0};
        auto w = [&]() {
            (void)hipSetDevice(device);
            for (;;) { const size_t s = next.fetch_add(1); if (s >= S) break; if (n_bytes[s] && hipMemcpy(raw + R.s_beg[s], streams[s], n_bytes[s], hipMemcpyHostToDevice) != hipSuccess) bad.store(1); }
        };
        std::vector<std::thread> th;
        for (size_t k = 0; k < std::min<size_t>(S, 6); ++k) th.emplace_back(w);
        for (auto &x : th) x.join();
        if (bad.load()) return fail(MSNV_EHIP, "upload of the record streams failed: %s", hipGetErrorString(hipGetLastError()));
    }
    R.wall_upload_s += now_s() - t0;
    R.raw = raw;
    return MSNV_OK;
}

// SubWalk's out-of-line members (devrec.h): the settle template there is each route's, these are compiled here once
void SubWalk::take(BufPool &pool) {
    d_ss = pool.take<SubStream>(S);
    d_first = pool.take<unsigned long long>((uint64_t)n_sub + 1);
    d_stop = pool.take<unsigned long long>((uint64_t)n_sub + 1);
    d_stopmax = pool.take<unsigned long long>((uint64_t)n_sub + 1);
    d_cnt = pool.take<uint32_t>((uint64_t)n_sub + 1);
    d_delta = pool.take<uint16_t>((uint64_t)n_sub * cap + 8);
    d_fl = pool.take<uint32_t>(4);
    d_firstbad = pool.take<uint32_t>(S);
}
int SubWalk::upload(hipStream_t st, const std::vector<SubStream> &ss, const std::vector<unsigned long long> &s_end, unsigned long long *d_send) {
    HIP_TRY(hipMemcpyAsync(d_ss, ss.data(), S * sizeof(SubStream), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_send, s_end.data(), S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_fl, 0, 16, st));
    HIP_TRY(hipMemsetAsync(d_firstbad, 0xff, S * 4, st));
    return MSNV_OK;
}
int SubWalk::scan_stops(Prim &prim, size_t *ask) { return prim.inclusive(d_stop, d_stopmax, (size_t)n_sub, U64Max(), ask); }
void SubWalk::check_seams(hipStream_t st) {
    hipLaunchKernelGGL(msnv_scan_check, grid_for((uint64_t)n_sub + 1, 256), dim3(256), 0, st, d_ss, (uint32_t)S, n_sub, sub_bytes, d_first, d_stopmax, d_cnt, d_firstbad);
}

// Record boundaries of staged streams, the quick way: sub-segments walked side by side, seams checked on the device.  `found` says whether
// the walk stands; a chain that breaks or a sub-segment with more records than its slots leaves the round to scan_segments (counted).
static int scan_sub_walk(hipStream_t st, BufPool &pool, const uint64_t *n_bytes, const size_t S, const size_t NC, ScanResult &R, bool &found) {
    found = false;
    const uint32_t sub_bytes = knob::scan_sub_bytes(knob::SCAN_SUB_STREAMS);   // (per call: tests shrink it)
    std::vector<SubStream> ss(S);
    uint64_t n_sub64 = 0;
    for (size_t s = 0; s < S; ++s) { ss[s] = SubStream{R.s_beg[s], R.s_end[s], (uint32_t)n_sub64, 0u}; n_sub64 += std::max<uint64_t>(1, (n_bytes[s] + sub_bytes - 1) / sub_bytes); }
    if (n_sub64 >= 0x7ffffff0ull) return MSNV_OK;
    SubWalk W(S, (uint32_t)n_sub64, sub_bytes, sub_bytes / 36u + 2u);
    const uint32_t n_sub = W.n_sub;
    uint8_t *const raw = R.raw;
    Timer tm(st);
    Prim prim(st);
    const size_t pool_from = pool.mark();
    W.take(pool);
    auto *d_base = pool.take<uint32_t>((uint64_t)n_sub + 1);
    auto *d_recbase = pool.take<uint32_t>(S + 1);
    auto *d_send = pool.take<unsigned long long>(S);
    if (pool.rc) return pool.rc;
    if (int rc = prim.bind(pool, 1u << 20)) return rc;
    tm.start();
    if (int rc = W.upload(st, ss, R.s_end, d_send)) return rc;
    hipLaunchKernelGGL(msnv_scan_sub, grid_for(n_sub, 256), dim3(256), 0, st, raw, W.d_ss, (uint32_t)S, n_sub, sub_bytes, W.cap, (int)NC, W.d_first, W.d_stop, W.d_cnt, W.d_delta, W.d_fl);
    HIP_TRY(hipGetLastError());
    size_t need = 0;                                              // both scans' storage before either is queued
    if (int rc = W.scan_stops(prim, &need)) return rc;
    if (int rc = prim.exclusive(W.d_cnt, d_base, 0u, (size_t)n_sub + 1, rocprim::plus<uint32_t>(), &need)) return rc;
    if (int rc = prim.room(need)) return rc;
    uint32_t fl = 0;
    auto fix = [&]() {
        hipLaunchKernelGGL(msnv_scan_fix, grid_for(S, 64), dim3(64), 0, st, raw, W.d_ss, (uint32_t)S, sub_bytes, W.cap, W.d_first, W.d_stop, W.d_stopmax, W.d_cnt, W.d_delta, W.d_firstbad, W.d_fl);
    };
    if (int rc = W.settle(st, prim, fix, []() { return MSNV_OK; }, fl, R.n_redone)) return rc;
    if (fl) {
        R.ms_scan += tm.stop();
        R.n_redone += 1;                                          // (counted: the round goes through the careful kernel)
        pool.rewind(pool_from);
        return MSNV_OK;
    }
    if (int rc = prim.exclusive(W.d_cnt, d_base, 0u, (size_t)n_sub + 1, rocprim::plus<uint32_t>())) return rc;
    HIP_TRY(hipMemcpyAsync(&R.NR, d_base + n_sub, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (a 32-bit count that wrapped would show as a total below the sub-segments' sum; 2^32 records need 150 GB of stream in one round -- refused by size)
    if (R.raw_bytes / 36 > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 records in one round of the device pack");
    const uint32_t NR = R.NR;
    auto *d_recoff = pool.take<unsigned long long>((uint64_t)NR + 1);
    auto *d_recsample = pool.take<uint16_t>((uint64_t)NR + 1);
    if (pool.rc) return pool.rc;
    hipLaunchKernelGGL(msnv_scan_write, grid_for(n_sub, 256), dim3(256), 0, st, W.d_ss, (uint32_t)S, n_sub, sub_bytes, W.cap, W.d_cnt, d_base, W.d_delta, d_recoff, d_recsample, d_recbase);
    HIP_TRY(hipGetLastError());
    R.rec_base.assign(S + 1, 0);
    HIP_TRY(hipMemcpyAsync(d_recbase + S, &R.NR, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(R.rec_base.data(), d_recbase, S * 4, hipMemcpyDeviceToHost, st));
    R.ms_scan += tm.stop();                                       // (waits: both copies are done)
    R.rec_base[S] = NR;
    R.n_rec.assign(S, 0); R.bad_off.assign(S, ~0ull);
    for (size_t s = 0; s < S; ++s) R.n_rec[s] = R.rec_base[s + 1] - R.rec_base[s];
    R.d_recbase = d_recbase; R.d_send = d_send; R.d_recoff = d_recoff; R.d_recsample = d_recsample;
    found = true;
    return MSNV_OK;
}

// Record boundaries of staged streams, the careful way: segments, guessed entry points, seams checked on the host; words malformed input.
static int scan_segments(hipStream_t st, BufPool &pool, const size_t S, const size_t NC, ScanResult &R) {
    const std::vector<unsigned long long> &s_beg = R.s_beg, &s_end = R.s_end;
    uint8_t *const raw = R.raw;
    Timer tm(st);
    const uint64_t seg_bytes = knob::scan_seg_bytes();   // (per call: tests shrink it)
    std::vector<ScanSeg> segs;
    std::vector<uint32_t> seg_lo(S + 1, 0);                       // per stream: its first segment
    uint64_t cap_total = 0;
    for (size_t s = 0; s < S; ++s) {
        seg_lo[s] = (uint32_t)segs.size();
        for (uint64_t o = s_beg[s]; o < s_end[s]; o += seg_bytes) {
            const uint64_t e = std::min<uint64_t>(o + seg_bytes, s_end[s]);
            segs.push_back(ScanSeg{o, e, s_end[s], o == s_beg[s] ? o : ~0ull, cap_total});
            cap_total += (e - o) / 36 + 2;
        }
    }
    seg_lo[S] = (uint32_t)segs.size();
    const size_t NSEG = segs.size();
    if (NSEG > 0x7fffffffull) return fail(MSNV_EDOMAIN, "too many scan segments in one round");
    auto *d_segs = pool.take<ScanSeg>(NSEG + 1);
    auto *d_outs = pool.take<ScanOut>(NSEG + 1);
    auto *d_tmpoff = pool.take<unsigned long long>(cap_total + 64);
    if (pool.rc) return pool.rc;
    std::vector<ScanOut> outs(NSEG);
    std::vector<uint32_t> &n_rec = R.n_rec; n_rec.assign(S, 0); std::vector<uint32_t> acc_cnt(NSEG, 0);
    std::vector<unsigned long long> &bad_off = R.bad_off; bad_off.assign(S, ~0ull);
    tm.start();
    if (NSEG) {
        HIP_TRY(hipMemcpyAsync(d_segs, segs.data(), NSEG * sizeof(ScanSeg), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(msnv_scan_segments, dim3((unsigned)NSEG), dim3(64), 0, st, raw, d_segs, (uint32_t)NSEG, (int)NC, d_tmpoff, d_outs);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(outs.data(), d_outs, NSEG * sizeof(ScanOut), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // seams: cur = where the true chain stands; a segment is accepted when its walk began exactly there
        std::vector<unsigned long long> cur(S);
        std::vector<uint32_t> at(S);                             // next segment to look at, per stream
        for (size_t s = 0; s < S; ++s) { cur[s] = s_beg[s]; at[s] = seg_lo[s]; }
        const size_t repair_lists = pool.mark();                  // (the two lists below are reused by every repair round)
        for (int round_no = 0;; ++round_no) {
            std::vector<uint32_t> redo;
            for (size_t s = 0; s < S; ++s) {
                while (at[s] < seg_lo[s + 1] && bad_off[s] == ~0ull) {
                    const uint32_t k = at[s];
                    if (cur[s] >= segs[k].end) { acc_cnt[k] = 0; ++at[s]; continue; }          // a record runs across the whole segment
                    if (outs[k].first != cur[s]) { segs[k].start = cur[s]; redo.push_back(k); break; }
                    acc_cnt[k] = outs[k].cnt;
                    if (outs[k].bad != ~0ull) { bad_off[s] = outs[k].bad - s_beg[s]; break; }
                    cur[s] = outs[k].stop;
                    ++at[s];
                }
            }
            if (redo.empty()) break;
            if (round_no > (int)NSEG + 1) return fail(MSNV_EINVAL, "internal: the record scan does not converge");
            // walk the segments that guessed wrong again, from the true entry point (one launch over just those)
            std::vector<ScanSeg> again;
            for (uint32_t k : redo) again.push_back(segs[k]);
            auto *d_again = pool.take<ScanSeg>(again.size());
            auto *d_aout = pool.take<ScanOut>(again.size());
            if (pool.rc) return pool.rc;
            std::vector<ScanOut> aout(again.size());
            HIP_TRY(hipMemcpyAsync(d_again, again.data(), again.size() * sizeof(ScanSeg), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(msnv_scan_segments, dim3((unsigned)again.size()), dim3(64), 0, st, raw, d_again, (uint32_t)again.size(), (int)NC, d_tmpoff, d_aout);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(aout.data(), d_aout, again.size() * sizeof(ScanOut), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t j = 0; j < redo.size(); ++j) outs[redo[j]] = aout[j];
            R.n_redone += redo.size();
            pool.rewind(repair_lists);
        }
    }
    R.ms_scan += tm.stop();                                       // (the lists below are allocated outside the timed region)
    std::vector<uint32_t> &rec_base = R.rec_base; rec_base.assign(S + 1, 0);
    std::vector<CompactSeg> csegs;
    {
        uint64_t total = 0;
        for (size_t s = 0; s < S; ++s) {
            rec_base[s] = (uint32_t)total;
            for (uint32_t k = seg_lo[s]; k < seg_lo[s + 1]; ++k) {
                if (acc_cnt[k]) csegs.push_back(CompactSeg{segs[k].out_base, (uint32_t)total, acc_cnt[k], (uint32_t)s, 0u});
                total += acc_cnt[k];
                if (total > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 records in one round of the device pack");
            }
            n_rec[s] = (uint32_t)total - rec_base[s];
        }
        rec_base[S] = (uint32_t)total;
    }
    R.NR = rec_base[S];
    const uint64_t NRa = (uint64_t)R.NR + 1;
    R.d_recbase = pool.take<uint32_t>(S + 1);
    R.d_send = pool.take<unsigned long long>(S);
    R.d_recoff = pool.take<unsigned long long>(NRa);
    R.d_recsample = pool.take<uint16_t>(NRa);
    auto *d_csegs = pool.take<CompactSeg>(csegs.size() + 1);
    if (pool.rc) return pool.rc;
    tm.start();
    HIP_TRY(hipMemcpyAsync(R.d_recbase, rec_base.data(), (S + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(R.d_send, s_end.data(), S * 8, hipMemcpyHostToDevice, st));
    if (!csegs.empty()) {
        HIP_TRY(hipMemcpyAsync(d_csegs, csegs.data(), csegs.size() * sizeof(CompactSeg), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(msnv_compact_offsets, dim3((unsigned)csegs.size()), dim3(256), 0, st, d_tmpoff, d_csegs, R.d_recoff, R.d_recsample);
        HIP_TRY(hipGetLastError());
    }
    R.ms_scan += tm.stop();                                       // (waits: csegs' bytes are up)
    return MSNV_OK;
}
// Where the records of staged streams begin: the sub-segment walk, and the segment scan for what it leaves (and under MSNV_SCAN=segments).
int scan_records(hipStream_t st, BufPool &pool, const uint64_t *n_bytes, const size_t S, const size_t NC, ScanResult &R) {
    if (!knob::scan_segments() && S > 0) {
        bool found = false;
        if (int rc = scan_sub_walk(st, pool, n_bytes, S, NC, R, found)) return rc;
        if (found) return MSNV_OK;
    }
    return scan_segments(st, pool, S, NC, R);
}

// The runtime loads a translation unit's code object when its first kernel is launched: msnv_ctx_create does that (devpack.hip: warm_devpack).
__global__ void msnv_warm_devscan() {}
void warm_devscan(void *stream) { hipLaunchKernelGGL(msnv_warm_devscan, dim3(1), dim3(1), 0, (hipStream_t)stream); (void)hipGetLastError(); }

}  // namespace msnv
