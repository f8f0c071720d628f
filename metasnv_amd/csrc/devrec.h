// metasnv_amd/csrc/devrec.h -- a BAM record on the device and the sub-segment walk over a stream's records: what more than one of devscan.hip (the
// record scan), devdeal.hip (the dealer), devsub.hip (the read subsampler) and devpack.hip (the round of the per-read stage) inlines or declares
// (HIP only; no kernel lives here).
//   Rec, rec_load .. cg_match     the fixed part of an alignment record read from HBM, the CIGAR operations' classes
//   SubStream .. guess_entry      a stream's sub-segments: which bytes one holds, where the chain of records enters them (a guess)
//   scan_sub_body<Walk>, scan_fix_body<Walk>, chain_before     the bodies of the walk and the fix kernels over a Walk: WalkPlain (devscan.hip: offsets) or
//                                 WalkMeasure (devpack.hip: slots and sums); wave_records for the two kernels that write the records out in record order
//   ScanResult, stage_streams, scan_records     staged streams and the offsets of their records (devscan.hip): what a round and the dealer start from
//   SubWalk                       the walk's buffers and the seam loop on the host, for the record scan and the round's quick front
#pragma once

#include <vector>

#include "devwork.h"

namespace msnv {

// ------------------------------------------------------------------------------------------ a record
// fixed part of an alignment record (SAM spec 4.2): block_size refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen
struct Rec {
    int32_t tid, pos, l_seq, mtid, mpos, tlen;
    uint32_t bs, l_name, n_cigar, flag, mapq;
    const uint8_t *cigar, *seq, *qual;
    bool ok;
};
__device__ __forceinline__ Rec rec_load(const uint8_t *p, uint64_t avail) {
    Rec r;
    uint4 h0, h1; __builtin_memcpy(&h0, p, 16); __builtin_memcpy(&h1, p + 16, 16);      // (two 16-byte loads and a word instead of four 8-byte ones and a word: the walks that call this are bound by the NUMBER of memory requests)
    r.bs = h0.x; r.tid = (int32_t)h0.y; r.pos = (int32_t)h0.z;
    const uint32_t w = h0.w;
    r.l_name = w & 0xffu; r.mapq = (w >> 8) & 0xffu;
    const uint32_t fn = h1.x;
    r.n_cigar = fn & 0xffffu; r.flag = fn >> 16; r.l_seq = (int32_t)h1.y;
    r.mtid = (int32_t)h1.z; r.mpos = (int32_t)h1.w; r.tlen = (int32_t)ld32(p + 32);
    r.cigar = p + 36 + r.l_name;
    r.seq = r.cigar + 4ull * r.n_cigar;
    r.qual = r.seq + ((uint64_t)(uint32_t)r.l_seq + 1) / 2;
    const uint64_t need = 36ull + r.l_name + 4ull * r.n_cigar + ((uint64_t)(uint32_t)r.l_seq + 1) / 2 + (uint64_t)(uint32_t)r.l_seq;
    r.ok = avail >= 36 && (int32_t)r.bs >= 32 && (uint64_t)r.bs + 4 <= avail && r.l_seq >= 0 && need <= (uint64_t)r.bs + 4;      // hostio.cpp: rec_parse
    // a CIGAR that lives in the CG:B,I field behind a placeholder `<l_seq>S<ref_len>N` (more than 65535 operations; sam.c bam_tag2cigar
    // [EXT]): the walk below is taken by such records only (hostio.cpp: rec_parse states the conditions)
    if (r.ok && r.n_cigar > 0 && r.tid >= 0 && r.pos >= 0) {
        const uint32_t c0 = ld32(r.cigar);
        if ((c0 & 15u) == C_S && (int32_t)(c0 >> 4) == r.l_seq) {
            const uint8_t *aux = r.qual + (uint32_t)r.l_seq, *end = p + 4ull + r.bs;
            while (aux + 3 <= end) {
                const uint8_t t = aux[2], *v = aux + 3;
                unsigned long long sz;
                if (t == 'A' || t == 'c' || t == 'C') sz = 1;
                else if (t == 's' || t == 'S') sz = 2;
                else if (t == 'i' || t == 'I' || t == 'f') sz = 4;
                else if (t == 'd') sz = 8;
                else if (t == 'Z' || t == 'H') { const uint8_t *q = v; while (q < end && *q) ++q; sz = (unsigned long long)(q - v) + 1; }
                else if (t == 'B') {
                    if (v + 5 > end) break;
                    const unsigned long long es = (v[0] == 'c' || v[0] == 'C') ? 1 : (v[0] == 's' || v[0] == 'S') ? 2 : 4, n = ld32(v + 1);
                    if (aux[0] == 'C' && aux[1] == 'G') {
                        if ((v[0] == 'I' || v[0] == 'i') && n >= r.n_cigar && n < (1ull << 29) && v + 5 + 4 * n <= end) { r.cigar = v + 5; r.n_cigar = (uint32_t)n; }
                        break;
                    }
                    sz = 5 + es * n;
                } else break;
                if (aux[0] == 'C' && aux[1] == 'G') break;
                if (v + sz > end) break;
                aux = v + sz;
            }
        }
    }
    return r;
}
__device__ __forceinline__ bool rec_mapped(uint32_t flag, int32_t tid) { return !(flag & 4u) && tid >= 0; }

__device__ __forceinline__ bool cg_ref(uint32_t t) { return t == C_M || t == C_D || t == C_N || t == C_EQ || t == C_X; }
__device__ __forceinline__ bool cg_query(uint32_t t) { return t == C_M || t == C_I || t == C_S || t == C_EQ || t == C_X; }
__device__ __forceinline__ bool cg_match(uint32_t t) { return t == C_M || t == C_EQ || t == C_X; }

// ------------------------------------------------------------------------------------------ the sub-segment walk
// The chain of a stream's records, found by many short walks side by side (round 5).  A stream is cut into SUB-SEGMENTS of a few kilobytes, one LANE
// each: the lane guesses where the chain enters its bytes -- the first offset whose 36 header bytes are those of a plausible record (sizes
// consistent, contig ids in range, the read name's terminating NUL where l_read_name says) and whose two successors are too --, walks the
// ~20 records that start there and leaves their offsets (16-bit, relative to the sub-segment) in its slots.  A second kernel checks every
// seam on the device -- a sub-segment's walk must have begun exactly where the chain stood after the sub-segments before it (running maximum
// of the walks' ends) --, a scan of the accepted counts gives every sub-segment its first record, a third kernel writes the offsets out.
// One wait, for the record count.  A seam that does not hold (a wrong guess: a record longer than a sub-segment with something
// header-like inside) is repaired on the device: msnv_scan_check finds every stream's first such sub-segment, msnv_scan_fix walks it again
// from the true entry (below).  Only a chain that breaks from its true entry, or a sub-segment with more records than slots, sends the round
// through msnv_scan_segments (devscan.hip), which words the error.
struct SubStream { unsigned long long beg, end; uint32_t sub0, pad; };        // bytes [beg, end) of the round buffer, first sub-segment
__device__ __forceinline__ bool hdr_plausible(const uint8_t *raw, unsigned long long o, unsigned long long s_end, int n_contigs, uint32_t &bs_out) {
    if (s_end - o < 36) return false;
    const uint64_t a = ld64(raw + o);
    const uint32_t bs = (uint32_t)a; const int32_t tid = (int32_t)(a >> 32);
    bs_out = bs;
    if ((int32_t)bs < 32 || bs >= (1u << 28) || (unsigned long long)bs + 4 > s_end - o || tid < -1 || tid >= n_contigs) return false;
    const uint64_t b = ld64(raw + o + 8), c = ld64(raw + o + 16), d = ld64(raw + o + 24);
    const int32_t pos = (int32_t)(uint32_t)b, l_seq = (int32_t)(c >> 32), mtid = (int32_t)(uint32_t)d, mpos = (int32_t)(d >> 32);
    const uint32_t l_name = (uint32_t)(b >> 32) & 0xffu, n_cigar = (uint32_t)c & 0xffffu;
    if (pos < -1 || l_name < 1 || l_seq < 0 || mtid < -1 || mtid >= n_contigs || mpos < -1) return false;
    const unsigned long long need = 36ull + l_name + 4ull * n_cigar + ((unsigned long long)(uint32_t)l_seq + 1) / 2 + (unsigned long long)(uint32_t)l_seq;
    if (need > (unsigned long long)bs + 4) return false;
    // (a GUESS may be as strict as it likes -- a sub-segment without one is walked from the true entry by msnv_scan_fix.  More than 64 KB of
    // auxiliary fields and a read name that does not begin and end on a printable character are turned down: four bytes in front of a true
    // header the last qualities of the record before read as a block_size of millions, the true block_size as a contig number -- with the
    // 2 500 contigs of BASELINE configs[2] that passed every other test ~20 times per stream, a repair pass each)
    if ((unsigned long long)bs + 4 - need > 65536ull) return false;
    if (raw[o + 36 + l_name - 1] != 0) return false;
    if (l_name >= 2) { const uint8_t c0 = raw[o + 36], c1 = raw[o + 36 + l_name - 2]; if (c0 < 33 || c0 > 126 || c1 < 33 || c1 > 126) return false; }
    return true;
}
__device__ __forceinline__ uint32_t sub_stream_of(const SubStream *ss, uint32_t n_streams, uint32_t g) {        // last stream whose first sub-segment is at or before g
    uint32_t a = 0, b = n_streams;
    while (b - a > 1) { const uint32_t m = (a + b) / 2; if (ss[m].sub0 <= g) a = m; else b = m; }
    return a;
}
// Sub-segment g: its stream (si, S) and its bytes [b, e) of the round buffer.  sub_at when the stream is known, sub_of finds it.
struct Sub { SubStream S; uint32_t si; unsigned long long b, e; };
__device__ __forceinline__ Sub sub_at(const SubStream *ss, uint32_t si, uint32_t g, uint32_t sub_bytes) {
    Sub u; u.S = ss[si]; u.si = si;
    u.b = u.S.beg + (unsigned long long)(g - u.S.sub0) * sub_bytes; u.e = u.b + sub_bytes < u.S.end ? u.b + sub_bytes : u.S.end;
    return u;
}
__device__ __forceinline__ Sub sub_of(const SubStream *ss, uint32_t n_streams, uint32_t g, uint32_t sub_bytes) { return sub_at(ss, sub_stream_of(ss, n_streams, g), g, sub_bytes); }
// Where the chain enters [b, e), guessed: the first offset that is plausible with its two successors (~0: none)
__device__ __forceinline__ unsigned long long guess_entry(const uint8_t *raw, const SubStream &S, unsigned long long b, unsigned long long e, int n_contigs) {
    // sixteen offsets a step from 32 bytes in registers (a load per offset made the kernel L2-bound: every lane steps through its own
    // cache lines); block_size and refID of a candidate are looked at first -- almost nothing else passes them
    unsigned long long f = ~0ull;
    const unsigned long long a0 = b & ~15ull;                  // (aligned 16-byte pieces; the buffer is readable 256 bytes past the last stream)
    uint4 lo4 = *reinterpret_cast<const uint4 *>(raw + a0);
    for (unsigned long long base16 = a0; base16 < e && f == ~0ull; base16 += 16) {
        const uint4 hi4 = *reinterpret_cast<const uint4 *>(raw + base16 + 16);
        const uint32_t w[7] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z};
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t bs = __builtin_amdgcn_alignbyte(w[(k >> 2) + 1], w[k >> 2], k & 3u);
            const int32_t tid = (int32_t)__builtin_amdgcn_alignbyte(w[(k >> 2) + 2], w[(k >> 2) + 1], k & 3u);
            const unsigned long long o = base16 + k;
            if ((int32_t)bs < 32 || bs >= (1u << 28) || tid < -1 || tid >= n_contigs || o < b || o >= e || f != ~0ull) continue;
            uint32_t bs1 = 0;
            if (!hdr_plausible(raw, o, S.end, n_contigs, bs1)) continue;
            bool ok = true;
            unsigned long long o2 = o + 4ull + bs1;
            for (int d = 0; d < 2 && ok && o2 < S.end; ++d) { uint32_t b2 = 0; ok = hdr_plausible(raw, o2, S.end, n_contigs, b2); o2 += 4ull + b2; }
            if (ok) f = o;
        }
        lo4 = hi4;
    }
    return f;
}
// A Walk goes over one sub-segment's records.  Two exist: WalkPlain in devscan.hip (the offsets: the careful route, the dealer) and WalkMeasure
// in devpack.hip (the slots and the sub-segment's SubInfo: the quick route).  What the scan and the fix body ask of one:
//   walk(g, entry, b, e, s_end, cap, sums, n, off)   from `entry`, the records that start in [b, e): the first `cap` into sub-segment g's
//                                                    slots; leaves their number in n, the chain's next offset in off, and adds what it
//                                                    sums to `sums`; returns whether the chain held
//   Sums, none()                                     what a walk sums, and its empty value (WalkPlain: nothing)
//   keep(g, sums)                                    stores the sums of an ACCEPTED walk -- info[g] is written by the measuring walk only
// One lane per sub-segment: the entry (the stream's first byte, or a guess), the walk from it, the verdict.
template <typename Walk>
__device__ __forceinline__ void scan_sub_body(const uint8_t *raw, const SubStream *ss, uint32_t n_streams, uint32_t n_sub, uint32_t sub_bytes, uint32_t cap, int n_contigs,
                                              unsigned long long *first, unsigned long long *stop, uint32_t *cnt, uint32_t *flags, const Walk &wk) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_sub) return;
    const Sub u = sub_of(ss, n_streams, g, sub_bytes);
    const bool guessed = g != u.S.sub0;
    const unsigned long long f = guessed ? guess_entry(raw, u.S, u.b, u.e, n_contigs) : u.S.beg;
    uint32_t n = 0; unsigned long long off = f;
    bool ok = true;
    typename Walk::Sums sums = Walk::none();
    if (f != ~0ull) ok = wk.walk(g, f, u.b, u.e, u.S.end, cap, sums, n, off);
    ok = ok && n <= cap;
    if (!ok && guessed) { first[g] = ~0ull - 1ull; stop[g] = 0ull; cnt[g] = 0u; return; }      // a walk from a GUESSED entry that breaks: a wrong guess (the fix kernel walks again from the true one)
    first[g] = f; stop[g] = f != ~0ull ? off : 0ull; cnt[g] = n;
    wk.keep(g, sums);
    if (!ok) atomicOr(flags, 1u);                                   // a malformed chain from the stream's first byte (or more records than slots): the careful kernel / route reports or takes it
}
// seams: cur = where the chain stands in front of sub-segment g = the largest end of a walk before it (the stream's first byte for its first
// sub-segment: ends of earlier streams lie before it)
__device__ __forceinline__ unsigned long long chain_before(const Sub &u, const unsigned long long *stop_max, uint32_t g) {      // (g is not its stream's first sub-segment)
    const unsigned long long cur = stop_max[g - 1];
    return cur > u.S.beg ? cur : u.S.beg;
}
// One lane per stream: its first sub-segment that guessed wrong, walked again from where the chain stands.
template <typename Walk>
__device__ __forceinline__ void scan_fix_body(const SubStream *ss, uint32_t n_streams, uint32_t sub_bytes, uint32_t cap, unsigned long long *first, unsigned long long *stop,
                                              const unsigned long long *stop_max, uint32_t *cnt, uint32_t *first_bad, uint32_t *flags, const Walk &wk) {
    const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= n_streams) return;
    const uint32_t g = first_bad[si];
    first_bad[si] = 0xffffffffu;                                    // (for the next pass)
    if (g == 0xffffffffu) return;
    const Sub u = sub_at(ss, si, g, sub_bytes);
    const unsigned long long cur = chain_before(u, stop_max, g);
    atomicOr(flags, 2u);
    typename Walk::Sums sums = Walk::none();
    if (cur >= u.e) { first[g] = ~0ull; stop[g] = 0ull; cnt[g] = 0u; wk.keep(g, sums); return; }
    uint32_t n = 0; unsigned long long off = cur;
    if (!wk.walk(g, cur, u.b, u.e, u.S.end, cap, sums, n, off) || n > cap) { atomicOr(flags, 4u); return; }
    first[g] = cur; stop[g] = off; cnt[g] = n;
    wk.keep(g, sums);
}
// The records in record order: a wavefront takes 64 consecutive sub-segments (n_here of them exist), whose records [w of lane 0, j_hi) are
// consecutive in the list, 64 a step; record j finds its sub-segment among the wavefront's by bisection over the lanes' first records (w).
// EVERY lane calls per_record(j, owner lane) in EVERY step -- it may shuffle the owner's values to itself, and a shuffle needs all lanes --,
// so per_record guards its own stores with j < j_hi.
template <typename PerRecord>
__device__ __forceinline__ void wave_records(uint32_t w, uint32_t n_here, uint32_t j_hi, PerRecord &&per_record) {
    const uint32_t lane = threadIdx.x & 63u, j_lo = __shfl(w, 0);
    for (uint32_t j0 = j_lo; j0 < j_hi; j0 += 64u) {
        const uint32_t j = j0 + lane;
        uint32_t lo = 0, hi = n_here;                              // last lane t (< n_here) whose first record is at or before j
#pragma unroll
        for (int it = 0; it < 6; ++it) {                           // (six halvings of at most 64 lanes; every lane takes every step: the shuffles need all lanes)
            const uint32_t m = (lo + hi) / 2;
            const uint32_t bm = __shfl(w, (int)m);
            if (hi - lo > 1) { if (bm <= j) lo = m; else hi = m; }
        }
        per_record(j, lo);
    }
}

// ------------------------------------------------------------------------------------------ host side (devscan.hip)
// Record streams (host or device memory) side by side in one device buffer and the offsets of their records: what the device pack
// (devpack_add_round) and the device dealer (msnv_records_deal_device) start from.
struct ScanResult {
    uint8_t *raw = nullptr; uint64_t raw_bytes = 0;
    std::vector<unsigned long long> s_beg, s_end, bad_off;      // per stream: first / end byte in raw; offset of a malformed record (~0: none)
    std::vector<uint32_t> rec_base, n_rec;                       // per stream: index of its first record / its record count
    uint32_t NR = 0;
    uint32_t *d_recbase = nullptr; unsigned long long *d_send = nullptr, *d_recoff = nullptr; uint16_t *d_recsample = nullptr;
    double wall_upload_s = 0, ms_scan = 0; uint64_t n_redone = 0;
};
// The round's streams side by side in one buffer: every stream starts on 16 bytes, readable bytes behind the last.  Nothing is scanned.
int stage_streams(hipStream_t st, const int device, BufPool &pool, const uint8_t *const *streams, const uint64_t *n_bytes, const size_t S, const bool on_device, ScanResult &R,
                  const uint8_t *in_place_base = nullptr);
// Where the records of staged streams begin: the sub-segment walk, and the segment scan for what it leaves (and under MSNV_SCAN=segments).
int scan_records(hipStream_t st, BufPool &pool, const uint64_t *n_bytes, const size_t S, const size_t NC, ScanResult &R);

// What the sub-segment walk of either route works on: the sub-segments' entries, ends, counts and offsets, the seam check's words.  A route
// adds its own buffers and kernels: the walk and the fix kernel, and what it queues behind the repair before the one wait.
struct SubWalk {
    uint32_t n_sub = 0, sub_bytes = 0, cap = 0; size_t S = 0;
    SubStream *d_ss = nullptr; unsigned long long *d_first = nullptr, *d_stop = nullptr, *d_stopmax = nullptr; uint32_t *d_cnt = nullptr; uint16_t *d_delta = nullptr;
    uint32_t *d_fl = nullptr, *d_firstbad = nullptr;
    SubWalk(size_t n_streams, uint32_t n_sub_, uint32_t sub_bytes_, uint32_t cap_) : n_sub(n_sub_), sub_bytes(sub_bytes_), cap(cap_), S(n_streams) {}
    void take(BufPool &pool);                                     // (the caller looks at pool.rc after its own takes)
    // the streams' sub-segments and ends up (d_send: the route's own copy of the ends), the flags cleared
    int upload(hipStream_t st, const std::vector<SubStream> &ss, const std::vector<unsigned long long> &s_end, unsigned long long *d_send);
    // settle's two steps that compile kernels, so defined once (devscan.hip): the running maximum of the walks' ends, d_stop -> d_stopmax (with
    // `ask` the storage query alone: Prim), and the msnv_scan_check launch
    int scan_stops(Prim &prim, size_t *ask = nullptr);
    void check_seams(hipStream_t st);
    // The seams, behind the walk kernel: checked, every stream's first sub-segment that guessed wrong walked again -- fix() launches the route's
    // fix kernel --, until none is left (usually the first look).  after() queues what the route wants behind the repair, so that every pass
    // has ONE wait.  Leaves the flag word in `fl` (0: every seam holds; else the walk does not stand) and counts the repair passes.
    template <typename Fix, typename After>
    int settle(hipStream_t st, Prim &prim, Fix fix, After after, uint32_t &fl, uint64_t &n_redone) {
        for (int pass = 0;; ++pass) {
            if (int rc = scan_stops(prim)) return rc;
            check_seams(st);
            fix();
            HIP_TRY(hipGetLastError());
            if (int rc = after()) return rc;
            HIP_TRY(hipMemcpyAsync(&fl, d_fl, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (!(fl & 2u) || (fl & 5u) || pass >= 4096) return MSNV_OK;
            n_redone += 1;                                        // (counted: a repair pass)
            HIP_TRY(hipMemsetAsync(d_fl, 0, 4, st));
        }
    }
};

}  // namespace msnv
