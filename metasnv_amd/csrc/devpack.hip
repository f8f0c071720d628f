// metasnv_amd/csrc/devpack.hip -- the per-read stage as device kernels: raw BAM alignment records in HBM -> packed read columns.  The record
// scan it starts from is devscan.hip, the device dealer (msnv_records_deal_device) devdeal.hip; what the three share is devrec.h.
//
// What it replaces: the read loop of the reference's tools, per record -- flag / MAPQ / duplicate filter and the walk over the CIGAR's M
// blocks of qaCompute (/root/reference/src/qaTools/qaCompute.cpp:441-593, the walk :530-552), and what `samtools mpileup` (call site
// /root/reference/metaSNV.py:160-165; bam_plcmd.c mplp_func, sam.c resolve_cigar2 [EXT], restated in SURVEY.md Appendix C) does with a
// record before its pileup is counted: --ff 0x704, -l overlap, start beyond the reference, -q, orphans, the CIGAR walk to aligned
// (M/=/X) segments, '=' -> reference base, and the -Q test of every base.  pack.cpp is the same stage on host threads (MSNV_PACK=host);
// the two produce the same columns byte for byte (tests/test_gpu_devpack.py).
//
// Stages of one round of samples (round 6; DESIGN.md section 3 has the table with the kernels' times), the function of each beside it
// (members of `Round`; devpack_add_round is their driver).  Round::stage (devscan.hip: stage_streams) puts the streams in place.  The QUICK route, the
// default -- Round::front_quick, then launch_emit and collect:
//   msnv_scan_sub2        one LANE per sub-segment of a few kilobytes of a stream: guesses where the block_size chain enters its bytes, walks the
//                         records that start there and MEASURES each as it goes (header, CIGAR geometry, the read filters of both tools,
//                         qaCompute's statistics, the pieces / seq bytes / M intervals the record will emit) into a 32-byte slot
//   msnv_scan_check / _fix2 / msnv_sub_bounds + ONE scan of the sub-segments' sums: the seams (SubWalk::settle), what crosses them, the round's totals
//                         -- the stage's one wait: the host sizes every buffer from them
//   msnv_scan_write2      the records' tables in record order: offsets, {position, end, contig, sample}, places before every record
//   msnv_depth2           pileup reads alive at every read start (mpileup -d, the depth bound of the tile index, the upper bound of a
//                         sample's base string: snpCall's token limit) from a window of the records in front; on the second stream
//   msnv_emit_block       a workgroup per 256 records, their bytes staged in LDS: piece headers, qaCompute's intervals, bases (nibble swap,
//                         '=' -> reference code), "quality below the -Q cutoff" flags, mismatch sampling of every 16th piece, in TILE order
//                         (the pieces a read leaves in the next tile are placed by counting); msnv_emit_block_slow takes what it lists
//                         -- Round::launch_emit, both routes; Round::collect waits for the small results and can hand the round to the careful route
//   the (sample, tile) pairs (Round::tile_pairs: by counting over the groups, or the rocPRIM sort) and the samples' host fields (Round::publish)
// The CAREFUL route -- Round::front_careful: scan_records (devscan.hip), then per pass
// measure (msnv_measure_reads), tables_and_depth (msnv_tables_from_measure, msnv_depth2), list_overlaps, sequential_edits (the host pre-pass:
// host_prepass_samples), a wait between the stages; then Round::edit_qualities (msnv_ovl_groups, msnv_token_*) -- takes the
// rounds the quick one leaves: paired reads, chains that break, the general tile-order sort -- and the three SEQUENTIAL edits of the host
// stage, all kernels now: the overlapping-mate quality tweak (msnv_ovl_*, round 4), mpileup's depth cap (msnv_cap_reads) and snpCall's token
// limit (msnv_token_clamp, msnv_token_cut; round 6).  Which samples' records can trigger one is decided on the device (a read starts above
// the cap; two or more reads pass htslib's overlap_push precondition; the upper bound of a base string reaches the limit).  The host
// pre-pass (pack.cpp: host_prepass) keeps three corner cases (a template with more alignments than the overlap kernel's slots, reads that
// span more than 16 384 reference positions, an indel of half a million bases) and MSNV_PREPASS=host.
// The sub-segment walk is written once for both routes and the dealer (devrec.h); this file's Walk is WalkMeasure (slots and sums).  AccAdd
// is what a record or a sub-segment adds to its sample's accumulators.
// Behind the round: devpack_sync_pending, the dataset's pinned block (pin_ensure), devpack_release, and the copies of a device-packed
// sample to host staging (devpack_download_pieces, devpack_sample_to_host).  Finalize's device side is devfin.hip; what the two files share
// -- HIP_TRY, DevBuf, BufPool, Prim, the device helpers of a piece's bytes -- is devwork.h, and the two kernels of the round that finalize's
// deep-run split borrows are behind devpack_gather_pieces / devpack_emit_tail at the end of this file.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "devfin.h"
#include "devrec.h"

namespace msnv {

namespace {

struct DpParams {
    int flag_filter, min_mapq, count_orphans, cov_min_mapq, max_depth, token_limit, ignore_overlaps;
    int c_eff, all_low;            // the -Q cutoff as finalize.cpp: pack_lowq applies it: flagged = all_low || quality < c_eff
    int n_contigs, has_bed;
};
// per sample of the round
struct DpAcc {
    unsigned long long err;         // min over records of (flat record index << 3 | kind), ~0 = none
    unsigned long long first_pile;  // min flat index of a read that enters the pileup
    unsigned long long beyond;      // min flat index of a read whose qaCompute cursor reaches the contig end
    unsigned long long n_bases, alg8d, alg_cigar, alg_seq, alg_qual, mm_bases, mm;
    uint32_t total, unmapped, zeroq, proper, dup, any_mapped;
    uint32_t n_pile_reads, n_ovl, need_host, pad;
};
// A sample's accumulators exist ACC_COPIES times (a workgroup adds to copy blockIdx % ACC_COPIES, msnv_acc_fold sums them into copy 0): a round
// of a few big samples -- BASELINE configs[2]: eight per round -- otherwise sends every wavefront's atomics to the same eight cache lines
// (the measure kernel ran 3.4 x slower per record there than on the benchmark's 160 samples a round).
constexpr uint32_t ACC_COPIES = 64;
enum : uint32_t { ERR_MALFORMED = 1, ERR_TID = 2, ERR_UNSORTED = 3, ERR_QLEN = 4 };
enum : uint8_t { RF_PILE = 1, RF_COV = 2, RF_MAPPED = 4, RF_OVL = 8 };      // RF_OVL: passes sam.c overlap_push's precondition (a mate may overlap it)
enum : uint32_t { NEED_CAP = 1, NEED_TOKEN = 2, NEED_OVL = 4, NEED_BIGC = 8 };      // NEED_OVL: too many alignments of one template wait at once for the device's slots; NEED_BIGC (with NEED_TOKEN):
                                                                                      // an element longer than the records' tables can say -- both are the host pre-pass's


__global__ __launch_bounds__(64) void msnv_acc_fold(DpAcc *acc, uint32_t n_samples) {       // one wavefront per sample, one lane per copy (ACC_COPIES = 64)
    const uint32_t s = blockIdx.x, c = threadIdx.x;
    if (s >= n_samples) return;
    DpAcc &b = acc[(size_t)s * ACC_COPIES + c];
    DpAcc v = b;
    auto mn = [](unsigned long long x) { for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(x, o); x = y < x ? y : x; } return x; };
    auto su = [](unsigned long long x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o); return x; };
    auto s32 = [](uint32_t x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o); return x; };
    auto o32 = [](uint32_t x) { for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o); return x; };
    DpAcc t;
    t.err = mn(v.err); t.first_pile = mn(v.first_pile); t.beyond = mn(v.beyond);
    t.n_bases = su(v.n_bases); t.alg8d = su(v.alg8d); t.alg_cigar = su(v.alg_cigar); t.alg_seq = su(v.alg_seq); t.alg_qual = su(v.alg_qual); t.mm_bases = su(v.mm_bases); t.mm = su(v.mm);
    t.total = s32(v.total); t.unmapped = s32(v.unmapped); t.zeroq = s32(v.zeroq); t.proper = s32(v.proper); t.dup = s32(v.dup); t.any_mapped = o32(v.any_mapped);
    t.n_pile_reads = s32(v.n_pile_reads); t.n_ovl = s32(v.n_ovl); t.need_host = o32(v.need_host); t.pad = 0;
    DpAcc z{}; z.err = z.first_pile = z.beyond = ~0ull;
    b = c == 0 ? t : z;                                          // (a copy that has been folded in counts nothing twice)
}

__global__ void msnv_acc_init(DpAcc *acc, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DpAcc z{}; z.err = z.first_pile = z.beyond = ~0ull;
    acc[i] = z;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                   // lane 0
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_down(v, o); v = w < v ? w : v; }
    return v;
}
// What some records add to their sample's DpAcc: one record's (a lane of msnv_measure_reads), one sub-segment's (a lane of msnv_scan_write2),
// or -- acc_wave, in lane 0 -- a wavefront's, when all of it is one sample's.  The caller picks the copy (ACC_COPIES) that acc_add adds to.
struct AccAdd {
    uint32_t total = 0, unmapped = 0, zeroq = 0, proper = 0, dup = 0, any_mapped = 0, n_pile_reads = 0, n_ovl = 0;
    unsigned long long n_bases = 0, alg8d = 0, alg_cigar = 0, alg_seq = 0, alg_qual = 0;
    unsigned long long err = ~0ull, first_pile = ~0ull, beyond = ~0ull;        // minima (~0: none)
};
__device__ __forceinline__ AccAdd acc_wave(const AccAdd &x) {
    AccAdd t;
    t.total = wave_sum(x.total); t.unmapped = wave_sum(x.unmapped); t.zeroq = wave_sum(x.zeroq); t.proper = wave_sum(x.proper); t.dup = wave_sum(x.dup);
    t.any_mapped = wave_sum(x.any_mapped); t.n_pile_reads = wave_sum(x.n_pile_reads); t.n_ovl = wave_sum(x.n_ovl);
    t.n_bases = wave_sum(x.n_bases); t.alg8d = wave_sum(x.alg8d); t.alg_cigar = wave_sum(x.alg_cigar); t.alg_seq = wave_sum(x.alg_seq); t.alg_qual = wave_sum(x.alg_qual);
    t.err = wave_min(x.err); t.first_pile = wave_min(x.first_pile); t.beyond = wave_min(x.beyond);
    return t;
}
__device__ __forceinline__ void acc_add(DpAcc &a, const AccAdd &x) {       // (an atomic only where there is something to add: most counters of most wavefronts are zero)
    if (x.total) atomicAdd(&a.total, x.total);
    if (x.unmapped) atomicAdd(&a.unmapped, x.unmapped);
    if (x.zeroq) atomicAdd(&a.zeroq, x.zeroq);
    if (x.proper) atomicAdd(&a.proper, x.proper);
    if (x.dup) atomicAdd(&a.dup, x.dup);
    if (x.any_mapped) atomicOr(&a.any_mapped, 1u);
    if (x.n_pile_reads) atomicAdd(&a.n_pile_reads, x.n_pile_reads);
    if (x.n_ovl) atomicAdd(&a.n_ovl, x.n_ovl);
    if (x.n_bases) atomicAdd(&a.n_bases, x.n_bases);
    if (x.alg8d) atomicAdd(&a.alg8d, x.alg8d);
    if (x.alg_cigar) atomicAdd(&a.alg_cigar, x.alg_cigar);
    if (x.alg_seq) atomicAdd(&a.alg_seq, x.alg_seq);
    if (x.alg_qual) atomicAdd(&a.alg_qual, x.alg_qual);
    if (x.err != ~0ull) atomicMin(&a.err, x.err);
    if (x.first_pile != ~0ull) atomicMin(&a.first_pile, x.first_pile);
    if (x.beyond != ~0ull) atomicMin(&a.beyond, x.beyond);
}

// ------------------------------------------------------------------------------------------ per-record measure
// What a record adds to the running sums every later stage places things by: ONE exclusive scan of these over the round's records gives a
// record its rank among the pileup reads, its first piece, its first interval, the pieces earlier reads leave in the tile behind their
// own (tile order, below) and its first byte of the seq column.
struct RecCnt { uint32_t pile, npiece, niv, spill; unsigned long long seqb; };
struct RecCntSum { __device__ __host__ RecCnt operator()(const RecCnt &a, const RecCnt &b) const { return RecCnt{a.pile + b.pile, a.npiece + b.npiece, a.niv + b.niv, a.spill + b.spill, a.seqb + b.seqb}; } };
enum : uint32_t { MISC_SORT = 0, MISC_SPAN = 1, MISC_NOUT = 2, MISC_OVERHANG = 3, MISC_WORDS = 4 };   // words of the round's flag block: [MISC_SORT] the pieces need the general tile-order sort;
                                                                   // [MISC_SPAN] longest reference span of an ordinary pileup read; [MISC_NOUT] reads listed as outliers (msnv_depth)
// The records of a round in blocks of PB = one wavefront: the kernels that go over the records hold a block per wavefront, a block's sums
// (blk_cnt) are written by the measure kernel, ONE small scan over the blocks gives every block its base (blk_pre), and a record's own
// place is that base plus the sums of the records before it in its block -- recomputed by whoever needs it, from the 24 bytes per record
// the measure kernel left (a rocPRIM scan of those structs over all 15 M records of the benchmark shape cost 1 ms of the pack).
constexpr uint32_t PB = 64;
constexpr uint32_t SPAN_OUT = 16384;                                // a pileup read that spans more reference than this is listed by itself (msnv_depth's window stays short); raised when a round holds many such reads
constexpr uint32_t CAP_OUT = 4096;                                  // ... at most this many per round
__device__ __forceinline__ RecCnt wave_sum_cnt(RecCnt v) {
    for (int o = 32; o > 0; o >>= 1) { v.pile += __shfl_xor(v.pile, o); v.npiece += __shfl_xor(v.npiece, o); v.niv += __shfl_xor(v.niv, o); v.spill += __shfl_xor(v.spill, o); v.seqb += __shfl_xor(v.seqb, o); }
    return v;
}
__device__ __forceinline__ RecCnt wave_excl_cnt(const RecCnt c) {           // sums of the lanes before this one
    RecCnt v = c;
    const int lane = (int)(threadIdx.x & 63u);
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(v.pile, o), b = __shfl_up(v.npiece, o), d = __shfl_up(v.niv, o), e = __shfl_up(v.spill, o); const unsigned long long f = __shfl_up(v.seqb, o);
        if (lane >= o) { v.pile += a; v.npiece += b; v.niv += d; v.spill += e; v.seqb += f; }
    }
    return RecCnt{v.pile - c.pile, v.npiece - c.npiece, v.niv - c.niv, v.spill - c.spill, v.seqb - c.seqb};
}
__device__ __forceinline__ RecCnt cnt_add(const RecCnt &a, const RecCnt &b) { return RecCnt{a.pile + b.pile, a.npiece + b.npiece, a.niv + b.niv, a.spill + b.spill, a.seqb + b.seqb}; }
// Everything of pack.cpp: filter_and_edit + pack_sample that one record decides by itself.
struct RecMeasure {
    uint32_t flags;                // RF_*
    uint32_t err;                  // 0, or ERR_MALFORMED / ERR_TID / ERR_QLEN
    uint32_t st;                   // qaCompute's statistics and the round's flags: ST_* bits
    unsigned long long key;        // contig << 32 | position of a mapped record
    uint32_t end, maxc, np, sb, niv, ftile, spill;
    uint32_t m_bases, a_seq, n_cigar;      // of a read that enters the pileup: aligned bases, its seq bytes without padding, CIGAR operations
    int32_t over_tid, over_end;    // a read whose pieces run past its contig (ST_OVERHANG)
};
enum : uint32_t { ST_UNMAPPED = 1, ST_ZEROQ = 2, ST_PROPER = 4, ST_DUP = 8, ST_ANY = 16, ST_OVL = 32, ST_BEYOND = 64, ST_SORT = 128, ST_OVERHANG = 256, ST_ORDER = 512, ST_SHIPS = 1024 };
// ovr: the host pre-pass's verdict for this record (0: none)
// ctg_cache / cached_tid (may be NULL): the contig row of the record the caller measured before -- a walk's records mostly share one
__device__ __forceinline__ RecMeasure measure_one(const Rec &r, const DpContig *ctg, const DpParams &P, uint32_t ov, DpContig *ctg_cache = nullptr, int32_t *cached_tid = nullptr) {
    RecMeasure m{};
    if (!r.ok) { m.err = ERR_MALFORMED; return m; }
    if (!rec_mapped(r.flag, r.tid)) { m.st = ST_UNMAPPED; return m; }                     // qaCompute.cpp:461-473
    m.st = ST_ANY;
    bool cov_ok = false;
    if ((int)r.mapq >= P.cov_min_mapq) {                                                  // qaCompute.cpp:518-526
        if (r.flag & 2u) m.st |= ST_PROPER;
        if (r.flag & 0x400u) m.st |= ST_DUP; else cov_ok = true;
    } else m.st |= ST_ZEROQ;
    m.flags = RF_MAPPED;
    m.key = (unsigned long long)(uint32_t)r.tid << 32 | (uint32_t)r.pos;
    if (r.tid >= P.n_contigs) { m.err = ERR_TID; return m; }
    m.st |= ST_ORDER;                                                                     // (coordinate order: checked by the caller, against the neighbours' keys)
    DpContig c;
    if (ctg_cache) { if (*cached_tid != r.tid) { *ctg_cache = ctg[r.tid]; *cached_tid = r.tid; } c = *ctg_cache; }
    else c = ctg[r.tid];
    if (!c.sel) return m;
    // ---- CIGAR geometry, pieces, qaCompute's intervals: one walk
    long long rlen = 0, qlen = 0, m_bases = 0, ins = 0, del = 0, rp = r.pos, pp = (long long)r.pos + 1;
    bool has_ref_op = false, beyond = false;
    uint32_t n_piece = 0, seqb = 0, n_iv = 0, ftile = 0, ltile = 0, n_spill = 0;
    long long m_end = 0;                                                                   // end of the last aligned block
    unsigned long long a_seq = 0;
    uint32_t k0 = 0;
    if (r.n_cigar > 0) { const uint32_t t = ld32(r.cigar) & 15u; if (t == C_S || t == C_H) k0 = 1; }
    for (uint32_t k = 0; k < r.n_cigar; ++k) {
        const uint32_t cg = ld32(r.cigar + 4ull * k), t = cg & 15u, l = cg >> 4;
        if (cg_ref(t)) { rlen += l; has_ref_op = true; }
        if (cg_query(t)) qlen += l;
        if (t == C_I) ins += l; else if (t == C_D) del = del > (long long)l ? del : (long long)l;
        if (k >= k0) {                                                                     // qaCompute.cpp:537-552
            // (round 6: only the intervals the coverage index KEEPS are counted and written -- qaCompute.cpp:544-549 clips an M block's end to L - 1,
            // so a block that starts at L - 1, or an empty one, adds and takes away at the same position: finalize used to filter those in a
            // pass of its own over all intervals, msnv_fin_cov_measure + a scan)
            if (t == C_M) { if (pp >= c.len) { beyond = true; n_iv += c.len >= 1; } else if (pp < c.len - 1 && l > 0u) ++n_iv; }
            pp += l;
        }
        if (cg_match(t)) {
            m_bases += l;
            for (uint32_t off = 0, n = 0; off < l; off += n) {                             // pieces never cross a tile (pack.cpp: pack_sample)
                const uint32_t to_tile = TILE - (uint32_t)((rp + off) % TILE);
                n = SEG_MAX < l - off ? SEG_MAX : l - off;
                n = n < to_tile ? n : to_tile;
                const uint32_t tl = (uint32_t)((rp + off) / TILE);
                if (!n_piece) ftile = tl;
                if (tl != ftile) ++n_spill;
                ltile = tl;
                ++n_piece; seqb += stored_bytes(n); a_seq += (n + 1u) / 2u;
            }
            rp += l; m_end = rp;
        } else if (cg_ref(t)) rp += l;
    }
    const long long endpos = (long long)r.pos + (rlen ? rlen : 1);                         // bam_endpos
    // ---- mpileup's read-level filters, in mplp_func's order
    bool pile_ok = !(r.flag & (uint32_t)P.flag_filter);
    if (pile_ok && P.has_bed) pile_ok = c.bed_beg < endpos && (long long)r.pos < c.bed_end;
    if (pile_ok && c.seq_len >= 0 && c.seq_len <= (long long)r.pos) pile_ok = false;
    if (pile_ok && (int)r.mapq < P.min_mapq) pile_ok = false;
    if (pile_ok && !P.count_orphans && (r.flag & 1u) && !(r.flag & 2u)) pile_ok = false;
    if (pile_ok && !has_ref_op) pile_ok = false;
    if (pile_ok && r.l_seq > 0 && qlen != (long long)r.l_seq) m.err = ERR_QLEN;
    if (ov & 1u) pile_ok = (ov >> 1) & 1u;                                                 // the host pre-pass has decided (depth cap)
    const long long absl = r.tlen < 0 ? -(long long)r.tlen : (long long)r.tlen;
    if (pile_ok && !P.ignore_overlaps && !(r.flag & 8u) && (r.flag & 2u) &&                 // sam.c overlap_push's precondition
        !((r.mtid >= 0 && r.tid != r.mtid) || (absl >= 2ll * r.l_seq && (long long)r.mpos >= endpos))) { m.st |= ST_OVL; m.flags |= RF_OVL; }
    const unsigned long long mc = 4ull + ((ins | del) ? 11ull + (unsigned long long)(ins > del ? ins : del) : 0ull);      // pack.cpp: max_element_chars
    m.maxc = (uint32_t)(mc < 0x7fffffffull ? mc : 0x7fffffffull);
    m.end = (uint32_t)(endpos < 0xffffffffll ? endpos : 0xffffffffll);
    if (cov_ok) { m.flags |= RF_COV; m.niv = n_iv; if (beyond) m.st |= ST_BEYOND; }
    if (pile_ok) {
        m.flags |= RF_PILE;
        m.m_bases = (uint32_t)m_bases; m.n_cigar = r.n_cigar;
        // SEQ '*' (l_seq = 0): N bases of quality 0, shipped only under -Q 0 (pack.cpp: pack_sample)
        if (r.l_seq > 0 || (P.c_eff == 0 && !P.all_low)) { m.np = n_piece; m.sb = seqb; m.a_seq = (uint32_t)a_seq; m.st |= ST_SHIPS; }
        // a read whose pieces run past its contig: the contig's tiles reach that far (finalize)
        if (m.np && m_end > c.len) { m.st |= ST_OVERHANG; m.over_tid = r.tid; m.over_end = (int32_t)(m_end < 0x7fffffffll ? m_end : 0x7fffffffll); }
        m.ftile = ftile; m.spill = m.np ? n_spill : 0u;
        // tile order by counting (msnv_emit_block) needs every pileup read to leave pieces in its first tile and at most the
        // one behind it; a read that reaches further (a reference skip, a read of thousands of bases) or ships no piece at all
        // sends the round through the general sort
        if (!m.np || ltile > ftile + 1u) m.st |= ST_SORT;
    }
    return m;
}
__global__ __launch_bounds__(256) void msnv_measure_reads(const uint8_t *raw, const unsigned long long *rec_off, const uint16_t *rec_sample, const uint32_t *rec_base,
                                                          const unsigned long long *s_end, uint32_t n_rec, const DpContig *ctg, DpParams P, const uint32_t *ovr,
                                                          uint8_t *r_flags, unsigned long long *r_key, uint32_t *r_end, uint32_t *r_maxc, RecCnt *r_cnt, uint32_t *r_ftile,
                                                          RecCnt *blk_cnt, DpAcc *acc, uint32_t *misc, uint32_t *outliers, uint32_t span_out, int32_t *overhang) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n_rec;
    const uint32_t s = valid ? rec_sample[i] : 0xffffffffu;
    AccAdd c;                                                       // what this record adds to its sample's accumulators
    uint8_t flags = 0; unsigned long long key = 0; uint32_t o_end = 0, o_maxc = 0, o_np = 0, o_sb = 0, o_niv = 0, o_ftile = 0, o_spill = 0;
    bool need_sort = false, order_me = false;
    if (valid) {
        const uint8_t *p = raw + rec_off[i];
        const Rec r = rec_load(p, s_end[s] - rec_off[i]);
        const RecMeasure m = measure_one(r, ctg, P, ovr ? ovr[i] : 0u);
        c.total = 1;
        if (m.err) c.err = (unsigned long long)i << 3 | m.err;
        c.unmapped = (m.st & ST_UNMAPPED) ? 1u : 0u; c.zeroq = (m.st & ST_ZEROQ) ? 1u : 0u; c.proper = (m.st & ST_PROPER) ? 1u : 0u; c.dup = (m.st & ST_DUP) ? 1u : 0u;
        c.any_mapped = (m.st & ST_ANY) ? 1u : 0u; c.n_ovl = (m.st & ST_OVL) ? 1u : 0u;
        flags = (uint8_t)m.flags; key = m.key; order_me = (m.st & ST_ORDER) != 0u;
        o_end = m.end; o_maxc = m.maxc; o_niv = m.niv; o_ftile = m.ftile; o_spill = m.spill; o_np = m.np; o_sb = m.sb;
        if (m.st & ST_BEYOND) c.beyond = i;
        if (m.flags & RF_PILE) {
            c.n_pile_reads = 1; c.first_pile = i;
            c.n_bases = m.m_bases;
            c.alg8d = 16ull + 4ull * m.n_cigar + ((unsigned long long)m.m_bases + 1) / 2 + (unsigned long long)m.m_bases;
            c.alg_cigar = 4ull * m.n_cigar;
            if (m.st & ST_SHIPS) { c.alg_seq = m.a_seq; c.alg_qual = m.m_bases; }
            if (m.st & ST_OVERHANG) { atomicMax(&overhang[m.over_tid], m.over_end); misc[MISC_OVERHANG] = 1u; }
            need_sort = (m.st & ST_SORT) != 0u;
        }
        r_flags[i] = flags; r_key[i] = key; r_end[i] = o_end; r_maxc[i] = o_maxc; r_ftile[i] = o_ftile;
    }
    {
        // coordinate order: against the MAPPED record before this one in its stream (unmapped ones -- placed mates -- are stepped over).  The
        // one before is nearly always a lane of this wavefront: its key comes by a shuffle; only a lane with no mapped record of its stream
        // in front of it in the wavefront goes back to the records themselves
        const unsigned long long mapped_m = __ballot((flags & RF_MAPPED) != 0);
        const uint32_t lane = threadIdx.x & 63u;
        const unsigned long long below = mapped_m & ((1ull << lane) - 1ull);
        const int src = below ? 63 - __builtin_clzll(below) : 0;
        const unsigned long long pk = __shfl(key, src); const uint32_t ps = __shfl(s, src);
        if (order_me) {
            bool have = below != 0ull && ps == s;
            unsigned long long prev_key = pk;
            if (!have) {
                const uint32_t stop = below ? i - (lane - (uint32_t)src) + 1u : i - lane;    // records of this wavefront in front of me were looked at (none mapped, or another stream's)
                for (uint32_t j = stop < rec_base[s] ? rec_base[s] : stop; j > rec_base[s];) {
                    --j;
                    const uint8_t *q = raw + rec_off[j];
                    const uint64_t a = ld64(q), c = ld64(q + 16);
                    const int32_t tj = (int32_t)(a >> 32);
                    if (!rec_mapped((uint32_t)c >> 16, tj)) continue;
                    prev_key = (unsigned long long)(uint32_t)tj << 32 | ld32(q + 8); have = true;
                    break;
                }
            }
            if (have) {
                const int32_t tj = (int32_t)(prev_key >> 32), pj = (int32_t)(uint32_t)prev_key, ti = (int32_t)(key >> 32), pi = (int32_t)(uint32_t)key;
                if (ti < tj || (ti == tj && pi < pj)) { const unsigned long long e = (unsigned long long)i << 3 | ERR_UNSORTED; c.err = e < c.err ? e : c.err; }
            }
        }
    }
    {
        const RecCnt mine = valid ? RecCnt{(flags & RF_PILE) ? 1u : 0u, o_np, o_niv, o_spill, (unsigned long long)o_sb} : RecCnt{};
        if (valid) r_cnt[i] = mine;
        const RecCnt tot = wave_sum_cnt(mine);
        if ((threadIdx.x & 63u) == 0 && valid) blk_cnt[i / PB] = tot;         // (i is a multiple of PB in lane 0: 256 threads = 4 blocks; the grid's last wavefronts may lie behind the last block)
        // reference span of the pileup reads: the depth kernel's window reaches that far back; a read far beyond the others' is listed by itself
        uint32_t span = (flags & RF_PILE) ? o_end - ((uint32_t)key & 0x7fffffffu) : 0u;
        if (span > span_out) { const uint32_t k = atomicAdd(&misc[MISC_NOUT], 1u); if (k < CAP_OUT) outliers[k] = i; span = 0; }
        for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(span, o); span = x > span ? x : span; }
        if ((threadIdx.x & 63u) == 0 && span > *(volatile uint32_t *)&misc[MISC_SPAN]) atomicMax(&misc[MISC_SPAN], span);      // (a plain look first: every wavefront's atomic on one word was 2 ms)
    }
    if (__any(need_sort) && (threadIdx.x & 63u) == 0) atomicOr(&misc[MISC_SORT], 1u);
    // ---- per-sample sums: a wavefront's records almost always belong to one sample -> one atomic per counter and wavefront
    const uint32_t s0 = __shfl(s, 0);
    const bool uniform = __all(s == s0 || !valid) && s0 != 0xffffffffu;
    if (uniform) {
        const AccAdd t = acc_wave(c);
        if ((threadIdx.x & 63u) == 0) acc_add(acc[(size_t)s0 * ACC_COPIES + (blockIdx.x % ACC_COPIES)], t);
    } else if (valid) acc_add(acc[(size_t)s * ACC_COPIES + (blockIdx.x % ACC_COPIES)], c);
}

// ------------------------------------------------------------------------------------------ depth at every read start
// pack.cpp keeps the pileup reads of a sample in a heap by reference end (sam.c bam_plp_push [EXT], sample-local): when a read starts,
// the ones that ended at or before its start are popped, then it is pushed -- depth = reads alive, itself included; the sum of their
// longest possible pileup elements bounds the sample's base string there (snpCall's token limit).  Here, without a sort (rounds 1-4 merged
// the starts and the ends of a round with a radix sort of 2 N keys): a read that is alive at the start p of read r began after p - W, W = the
// longest reference span of a read of the round: the reads alive at r are r itself and those of the WINDOW of reads of its run -- (sample,
// contig) -- that start in (p - W, p], before r, and end beyond p: a walk back over the records in front (msnv_depth2, below).  Reads that
// span more than SPAN_OUT positions (a reference skip; none in a metaSNV run) do not widen the window: they are few, listed by themselves
// and looked at by every read.
constexpr uint32_t DEPTH_BACK = 256;                               // records in front of a workgroup's 256 that msnv_depth2's LDS window holds (round 5: 768; 0.65 -> 0.60 ms)
struct DpRun { uint32_t sample; int32_t tid, first_any, first_from1; };
// The (run, first tile) groups: where a group's pieces lie in tile order -- [a, b) the pieces in its own tile, [b, end) the ones its reads
// leave in the tile behind -- and the depth bounds of the two parts, for the host; {pieces, next-tile pieces} before every group's first read
// (grp_pre; entry n_groups: the round's totals), for the kernels that place the headers.
struct DevGroupRec { uint32_t sample; int32_t tid; uint32_t tile, a, b, end, md_own, md_next; };
struct DpSampleDst { uint8_t *seq, *qual; unsigned long long pbase0; uint32_t cut_marks, pad; };      // where a sample's columns lie in the round's buffer, its first piece
// ------------------------------------------------------------------------------------------ round 6: scan and measure in ONE walk
// The quick scan's lane (one per sub-segment of a stream: devrec.h) has every record's header line in hand when it reads block_size; the
// measure kernel then went to the same lines again, one thread per record, for everything else (3.1 GB of sector fetches for the 3.07 GB of
// the benchmark's records, 0.92 ms + a wait).  Here the walk measures as it goes (measure_one) and leaves per RECORD a 32-byte slot -- key,
// end, flags, first tile and its places among the sub-segment's records: pieces, intervals, next-tile pieces, seq bytes, rank among the
// pileup reads, run and group starts before it -- and per SUB-SEGMENT its sums, qaCompute's statistics, the first / last pileup read and
// mapped record (what the neighbours' boundaries need) and the first error.  Seams are checked and wrong guesses walked again as before;
// msnv_sub_bounds settles what crosses a boundary (does the sub-segment's first pileup read start a run / a group?  is its first mapped
// record in order?); ONE scan over the sub-segments' sums gives every sub-segment its bases, and -- its last entry -- the round's totals:
// records, pileup reads, pieces, intervals, seq bytes, runs, groups.  That is the ONE wait of the stage: everything behind it
// (msnv_scan_write2: records in record order with GLOBAL places; depth; groups; layout; msnv_emit_block) is launched back to back.
struct Slot { uint4 a, b; };       // a = {pos, end, tid, maxc << 13 | inner group start << 8 | inner run start << 7 | err << 4 | RF_*}
                                   // b = {first tile, seq bytes before | pieces before << 16, intervals before | next-tile pieces before << 16,
                                   //      pileup reads before | inner run starts up to here << 8 | inner group starts up to here << 16}   (all inside the sub-segment)
struct SubCnt { uint32_t rec, pile, npiece, niv, spill, runs, grps, ovl; unsigned long long seqb; uint32_t sort, odd; };   // what ONE scan carries (48 B); ovl: reads that pass overlap_push's precondition;
                                                                   // sort: sub-segments that ask for the general tile-order sort; odd: ... that the quick route cannot take (a field of a slot overflows, two overhanging contigs)
struct SubCntSum { __device__ __host__ SubCnt operator()(const SubCnt &x, const SubCnt &y) const {
    return SubCnt{x.rec + y.rec, x.pile + y.pile, x.npiece + y.npiece, x.niv + y.niv, x.spill + y.spill, x.runs + y.runs, x.grps + y.grps, x.ovl + y.ovl, x.seqb + y.seqb, x.sort + y.sort, x.odd + y.odd}; } };
struct SubInfo {
    uint32_t pile, npiece, niv, spill, seqb;          // sums over the sub-segment's records
    uint32_t runs, grps;                              // run / group starts among its pileup reads, the FIRST one's not counted (msnv_sub_bounds settles that one)
    uint32_t fp_slot, fp_tid, fp_ftile, lp_tid, lp_ftile;       // first / last pileup read: slot (~0: none), contig, first tile
    uint32_t fm_slot; unsigned long long fm_key, lm_key;        // first / last MAPPED record (coordinate order across sub-segments); fm_slot ~0: none
    uint32_t st_unmapped, st_zeroq, st_proper, st_dup, st_any, st_ovl;
    uint32_t m_pile, alg8d, alg_cigar, alg_seq, alg_qual;
    uint32_t err;                                     // slot << 3 | kind of the first error (~0: none)
    uint32_t beyond_slot;                             // first record whose qaCompute cursor reaches the contig end (~0: none)
    uint32_t flags;                                   // 1: the pieces need the general tile-order sort; 2: a read runs past its contig (over_*); 4: ... past two different contigs; 8: a place inside the sub-segment does not fit its slot field
    int32_t over_tid, over_end;
    uint32_t maxc_big;                                // some pileup read's longest element does not fit the slot's 19 bits
};
constexpr uint32_t MAXC_SAT = 0x7ffffu;
// The measuring Walk: the chain, the slots, the sums.  The sums go straight into the SubInfo and live in registers through the walk:
// msnv_scan_sub2 takes 122 VGPRs, no scratch, no LDS, 4 waves per SIMD (MEASURED.md has the table).
struct WalkMeasure {
    typedef SubInfo Sums;
    const uint8_t *raw; const DpContig *ctg; const DpParams &P; uint16_t *delta; Slot *slots; SubInfo *info;
    static __device__ __forceinline__ SubInfo none() { SubInfo s{}; s.fp_slot = s.fm_slot = s.err = s.beyond_slot = 0xffffffffu; return s; }
    __device__ __forceinline__ bool walk(uint32_t g, unsigned long long entry, unsigned long long b, unsigned long long e, unsigned long long s_end, uint32_t cap, SubInfo &s,
                                         uint32_t &n, unsigned long long &off) const {
        uint16_t *dl = delta + (size_t)g * cap; Slot *sl = slots + (size_t)g * cap;
        DpContig c_cache{}; int32_t c_tid = -2;
        n = 0; off = entry;
        unsigned long long prev_key = 0; bool have_prev = false;                  // last mapped record of this walk
        uint32_t lp_sample_tid = 0, lp_ft = 0; bool have_lp = false;              // last pileup read of this walk
        while (off < e) {
            if (s_end - off < 36) return false;
            const Rec r = rec_load(raw + off, s_end - off);
            if ((int32_t)r.bs < 32 || (unsigned long long)r.bs + 4 > s_end - off) return false;
            if (n < cap) {
                const RecMeasure m = measure_one(r, ctg, P, 0u, &c_cache, &c_tid);
                uint32_t err = m.err;
                if (m.st & ST_ORDER) {                                             // coordinate order inside the walk (across sub-segments: msnv_sub_bounds)
                    if (have_prev) {
                        const int32_t tj = (int32_t)(prev_key >> 32), pj = (int32_t)(uint32_t)prev_key, ti = (int32_t)(m.key >> 32), pi = (int32_t)(uint32_t)m.key;
                        if ((ti < tj || (ti == tj && pi < pj)) && (!err || err > ERR_UNSORTED)) err = ERR_UNSORTED;      // (pack.cpp looks at the order before CIGAR against SEQ: the lower kind, as at a seam and in msnv_measure_reads)
                    }
                }
                if (m.flags & RF_MAPPED) {
                    if (s.fm_slot == 0xffffffffu) { s.fm_slot = n; s.fm_key = m.key; }
                    s.lm_key = m.key; prev_key = m.key; have_prev = true;
                }
                uint32_t run_start = 0, grp_start = 0;
                if (m.flags & RF_PILE) {
                    const uint32_t t = (uint32_t)(m.key >> 32);
                    if (!have_lp) { s.fp_slot = n; s.fp_tid = t; s.fp_ftile = m.ftile; }
                    else {
                        run_start = t != lp_sample_tid ? 1u : 0u;
                        grp_start = (run_start || m.ftile != lp_ft) ? 1u : 0u;
                        if (!run_start && lp_ft > m.ftile) s.flags |= 1u;           // (a read whose first aligned base lies in an earlier tile than its predecessor's: leading deletions)
                    }
                    lp_sample_tid = t; lp_ft = m.ftile; have_lp = true;
                    s.lp_tid = t; s.lp_ftile = m.ftile;
                    s.runs += run_start; s.grps += grp_start;
                }
                if (err && s.err == 0xffffffffu) s.err = n << 3 | err;
                if ((m.st & ST_BEYOND) && s.beyond_slot == 0xffffffffu) s.beyond_slot = n;
                if (m.st & ST_SORT) s.flags |= 1u;
                if (m.st & ST_OVERHANG) {
                    if ((s.flags & 2u) && s.over_tid != m.over_tid) s.flags |= 4u;
                    if (!(s.flags & 2u) || m.over_end > s.over_end) { s.over_tid = m.over_tid; s.over_end = m.over_end; }
                    s.flags |= 2u;
                }
                const uint32_t mc = m.maxc < MAXC_SAT ? m.maxc : MAXC_SAT;
                if ((m.flags & RF_PILE) && m.maxc >= MAXC_SAT) s.maxc_big = 1u;
                Slot q;
                q.a = make_uint4((uint32_t)m.key, m.end, (uint32_t)(m.key >> 32), mc << 13 | grp_start << 8 | run_start << 7 | (err & 7u) << 4 | (m.flags & 15u));
                q.b = make_uint4(m.ftile, s.seqb | s.npiece << 16, s.niv | s.spill << 16, s.pile | s.runs << 8 | s.grps << 16);
                sl[n] = q;
                dl[n] = (uint16_t)(off - b);
                // ---- the sub-segment's sums
                if (m.st & ST_UNMAPPED) s.st_unmapped += 1u;
                if (m.st & ST_ZEROQ) s.st_zeroq += 1u;
                if (m.st & ST_PROPER) s.st_proper += 1u;
                if (m.st & ST_DUP) s.st_dup += 1u;
                if (m.st & ST_ANY) s.st_any += 1u;
                if (m.st & ST_OVL) s.st_ovl += 1u;
                if (m.flags & RF_PILE) {
                    s.pile += 1u; s.m_pile += m.m_bases;
                    s.alg8d += 16u + 4u * m.n_cigar + (m.m_bases + 1u) / 2u + m.m_bases; s.alg_cigar += 4u * m.n_cigar;
                    if (m.st & ST_SHIPS) { s.alg_seq += m.a_seq; s.alg_qual += m.m_bases; }
                }
                s.npiece += m.np; s.niv += m.niv; s.spill += m.spill; s.seqb += m.sb;
                if ((s.npiece | s.niv | s.spill | s.seqb) > 0xffffu || s.pile > 0xffu) s.flags |= 8u;      // (a SEQ-less read with a CIGAR of thousands of bases, sub-segments of many kilobytes: the careful route's)
            }
            ++n;
            off += 4ull + r.bs;
        }
        return true;
    }
    __device__ __forceinline__ void keep(uint32_t g, const SubInfo &s) const { info[g] = s; }
};
__global__ __launch_bounds__(256) void msnv_scan_sub2(const uint8_t *raw, const SubStream *ss, uint32_t n_streams, uint32_t n_sub, uint32_t sub_bytes, uint32_t cap, int n_contigs,
                                                      const DpContig *ctg, DpParams P, unsigned long long *first, unsigned long long *stop, uint32_t *cnt, uint16_t *delta, Slot *slots, SubInfo *info,
                                                      uint32_t *flags) {
    scan_sub_body(raw, ss, n_streams, n_sub, sub_bytes, cap, n_contigs, first, stop, cnt, flags, WalkMeasure{raw, ctg, P, delta, slots, info});
}
__global__ void msnv_scan_fix2(const uint8_t *raw, const SubStream *ss, uint32_t n_streams, uint32_t sub_bytes, uint32_t cap, const DpContig *ctg, DpParams P, unsigned long long *first,
                               unsigned long long *stop, const unsigned long long *stop_max, uint32_t *cnt, uint16_t *delta, Slot *slots, SubInfo *info, uint32_t *first_bad, uint32_t *flags) {
    scan_fix_body(ss, n_streams, sub_bytes, cap, first, stop, stop_max, cnt, first_bad, flags, WalkMeasure{raw, ctg, P, delta, slots, info});
}
// What crosses a sub-segment's front boundary, once every seam holds: does its first pileup read start a run / a group (against the last
// pileup read of the nearest sub-segment of its stream in front of it that has one)?  is its first mapped record in coordinate order behind
// the last mapped one in front?  Output: the scan's input.
__global__ __launch_bounds__(256) void msnv_sub_bounds(const SubStream *ss, uint32_t n_streams, uint32_t n_sub, const uint32_t *cnt, SubInfo *info, SubCnt *out, uint8_t *bflag) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_sub) return;
    if (g == n_sub) { out[g] = SubCnt{}; return; }
    const uint32_t n = cnt[g];
    SubCnt c{};
    uint32_t bf = 0;
    if (n) {
        SubInfo I = info[g];
        const SubStream S = ss[sub_stream_of(ss, n_streams, g)];    // (the stream alone: no bytes are looked at here)
        if (I.fp_slot != 0xffffffffu) {
            bool have = false; uint32_t pt = 0, pf = 0;
            for (uint32_t k = g; k > S.sub0 && !have;) { --k; if (cnt[k] && info[k].fp_slot != 0xffffffffu) { have = true; pt = info[k].lp_tid; pf = info[k].lp_ftile; } }
            const bool run = !have || pt != I.fp_tid, grp = run || pf != I.fp_ftile;
            bf = (run ? 1u : 0u) | (grp ? 2u : 0u);
            if (!run && pf > I.fp_ftile) bf |= 4u;                   // (tile order needs the sort)
        }
        if (I.fm_slot != 0xffffffffu) {
            bool have = false; unsigned long long pk = 0;
            for (uint32_t k = g; k > S.sub0 && !have;) { --k; if (cnt[k] && info[k].fm_slot != 0xffffffffu) { have = true; pk = info[k].lm_key; } }
            if (have) {
                const int32_t tj = (int32_t)(pk >> 32), pj = (int32_t)(uint32_t)pk, ti = (int32_t)(I.fm_key >> 32), pi = (int32_t)(uint32_t)I.fm_key;
                if (ti < tj || (ti == tj && pi < pj)) { const uint32_t e = I.fm_slot << 3 | ERR_UNSORTED; if (e < I.err) info[g].err = e; }      // (an error AT the slot itself, if any, was there first: it keeps its word)
            }
        }
        c.rec = n; c.pile = I.pile; c.npiece = I.npiece; c.niv = I.niv; c.spill = I.spill; c.seqb = I.seqb;
        c.runs = I.runs + (bf & 1u); c.grps = I.grps + ((bf >> 1) & 1u);
        c.ovl = I.st_ovl; c.sort = ((I.flags & 1u) || (bf & 4u)) ? 1u : 0u; c.odd = (I.flags & 12u) ? 1u : 0u;
    }
    out[g] = c; bflag[g] = (uint8_t)bf;
}
// The records in record order, a wavefront per 64 consecutive sub-segments (wave_records): offsets, samples, and from the slots +
// the sub-segments' bases every record's row of the per-record tables.  The lane that holds a sub-segment adds its statistics to its
// sample's accumulators first (one atomic per counter and wavefront when the 64 sub-segments are one stream's, as nearly always).
struct RdTables {
    unsigned long long *rec_off; uint16_t *rec_sample; uint32_t *rec_base;
    uint4 *rd;                     // {position, end, contig, sample | outlier << 12 | longest pileup element << 13}
    RecCnt *r_pre;                 // places BEFORE the record (entry n_rec: the round's totals)
    uint32_t *r_ftile; uint8_t *r_flags; unsigned long long *r_rg;      // r_flags: RF_* | RF_RUN | RF_GRP; r_rg: run << 32 | group of a pileup read (1-based)
    uint32_t *run_first, *grp_first;                                    // (msnv_scan_write2 only; may be NULL) first record of every run / group
};
enum : uint8_t { RF_RUN = 16, RF_GRP = 32 };
__global__ __launch_bounds__(256) void msnv_scan_write2(const SubStream *ss, uint32_t n_streams, uint32_t n_sub, uint32_t sub_bytes, uint32_t cap, const uint32_t *cnt, const SubCnt *base,
                                                        const uint8_t *bflag, const uint16_t *delta, const Slot *slots, const SubInfo *info, RdTables T, DpAcc *acc, uint32_t *misc,
                                                        uint32_t *outliers, uint32_t span_out, int32_t *overhang, DpParams P) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u, g0 = g - lane;
    if (g0 >= n_sub) return;
    const bool have = g < n_sub;
    uint32_t si = 0xffffffffu, w = 0xffffffffu; unsigned long long b = 0;
    SubCnt B{}; uint32_t bf = 0, fp_slot = 0xffffffffu;
    {
        // ---- this lane's sub-segment: base, statistics, first error
        AccAdd c; uint32_t need = 0;
        if (have) {
            const Sub u = sub_of(ss, n_streams, g, sub_bytes);
            si = u.si; b = u.b;
            B = base[g]; w = B.rec; bf = bflag[g];
            if (g == u.S.sub0) T.rec_base[si] = w;
            if (cnt[g]) {
                const SubInfo I = info[g];
                fp_slot = I.fp_slot;
                c.total = cnt[g]; c.unmapped = I.st_unmapped; c.zeroq = I.st_zeroq; c.proper = I.st_proper; c.dup = I.st_dup; c.any_mapped = I.st_any; c.n_pile_reads = I.pile; c.n_ovl = I.st_ovl;
                c.n_bases = I.m_pile; c.alg8d = I.alg8d; c.alg_cigar = I.alg_cigar; c.alg_seq = I.alg_seq; c.alg_qual = I.alg_qual;
                if (I.err != 0xffffffffu) c.err = (unsigned long long)(w + (I.err >> 3)) << 3 | (I.err & 7u);
                if (I.fp_slot != 0xffffffffu) c.first_pile = w + I.fp_slot;
                if (I.beyond_slot != 0xffffffffu) c.beyond = w + I.beyond_slot;
                if ((I.flags & 1u) || (bf & 4u)) atomicOr(&misc[MISC_SORT], 1u);
                if (I.flags & 2u) { atomicMax(&overhang[I.over_tid], I.over_end); misc[MISC_OVERHANG] = 1u; }
                if (I.flags & 4u) misc[MISC_OVERHANG] = 2u;             // (two contigs' worth in one sub-segment: the host takes the careful route)
                if (I.maxc_big && P.token_limit > 0) need |= NEED_TOKEN | NEED_BIGC;      // (an element longer than the slot holds: the host pre-pass counts exactly)
            }
        }
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)si);
        if (__all(si == s0 || !have) && s0 != 0xffffffffu) {
            const AccAdd t = acc_wave(c);
            uint32_t nd = need; for (int o = 32; o > 0; o >>= 1) nd |= __shfl_down(nd, o);
            if (lane == 0) {
                acc_add(acc[(size_t)s0 * ACC_COPIES + ((blockIdx.x * 4u + (threadIdx.x >> 6)) % ACC_COPIES)], t);
                if (nd) atomicOr(&acc[(size_t)s0 * ACC_COPIES].need_host, nd);
            }
        } else if (have && c.total) {
            acc_add(acc[(size_t)si * ACC_COPIES + (blockIdx.x % ACC_COPIES)], c);
            if (need) atomicOr(&acc[(size_t)si * ACC_COPIES].need_host, need);
        }
    }
    // ---- the records of the wavefront's sub-segments, 64 at a time
    const uint32_t n_here = (n_sub - g0 < 64u ? n_sub - g0 : 64u);
    const uint32_t j_hi = base[g0 + n_here].rec;                    // (base has n_sub + 1 entries)
    uint32_t span_max = 0;
    wave_records(w, n_here, j_hi, [&](uint32_t j, uint32_t lo) {
        const uint32_t wt = __shfl(w, (int)lo), st = __shfl(si, (int)lo), bft = __shfl(bf, (int)lo), fpt = __shfl(fp_slot, (int)lo);
        const unsigned long long bt = __shfl(b, (int)lo);
        const uint32_t p_pile = __shfl(B.pile, (int)lo), p_np = __shfl(B.npiece, (int)lo), p_niv = __shfl(B.niv, (int)lo), p_sp = __shfl(B.spill, (int)lo), p_runs = __shfl(B.runs, (int)lo), p_grps = __shfl(B.grps, (int)lo);
        const unsigned long long p_seqb = __shfl(B.seqb, (int)lo);
        if (j < j_hi) {
            const uint32_t k = j - wt;
            const size_t sl = (size_t)(g0 + lo) * cap + k;
            const Slot q = slots[sl];
            T.rec_off[j] = bt + delta[sl]; T.rec_sample[j] = (uint16_t)st;
            uint8_t fl = (uint8_t)(q.a.w & 15u);
            const uint32_t mc = q.a.w >> 13;
            uint32_t outl = 0;
            if (fl & RF_PILE) {
                const uint32_t span = q.a.y - (q.a.x & 0x7fffffffu);
                if (span > span_out) { const uint32_t o = atomicAdd(&misc[MISC_NOUT], 1u); if (o < CAP_OUT) outliers[o] = j; outl = 1u; }
                else span_max = span > span_max ? span : span_max;
                const bool first_pile = k == fpt;
                const uint32_t run_s = first_pile ? (bft & 1u) : (q.a.w >> 7) & 1u, grp_s = first_pile ? (bft >> 1) & 1u : (q.a.w >> 8) & 1u;
                if (run_s) fl |= RF_RUN;
                if (grp_s) fl |= RF_GRP;
                // inclusive numbers: the starts before the sub-segment, its first pileup read's (settled at the boundary), the inner ones up to here
                const uint32_t run_no = p_runs + (bft & 1u) + ((q.b.w >> 8) & 0xffu), grp_no = p_grps + ((bft >> 1) & 1u) + ((q.b.w >> 16) & 0xffu);
                T.r_rg[j] = (unsigned long long)run_no << 32 | grp_no;
                if (run_s && T.run_first) T.run_first[run_no - 1u] = j;
                if (grp_s && T.grp_first) T.grp_first[grp_no - 1u] = j;
            }
            T.rd[j] = make_uint4(q.a.x, q.a.y, q.a.z, (st & 0xfffu) | outl << 12 | mc << 13);
            RecCnt pre;
            pre.pile = p_pile + (q.b.w & 0xffu); pre.npiece = p_np + (q.b.y >> 16); pre.niv = p_niv + (q.b.z & 0xffffu); pre.spill = p_sp + (q.b.z >> 16); pre.seqb = p_seqb + (q.b.y & 0xffffu);
            T.r_pre[j] = pre;
            T.r_ftile[j] = q.b.x; T.r_flags[j] = fl;
        }
    });
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(span_max, o); span_max = x > span_max ? x : span_max; }
    if (lane == 0 && span_max > *(volatile uint32_t *)&misc[MISC_SPAN]) atomicMax(&misc[MISC_SPAN], span_max);
    // (entry n_rec of r_pre / rec_off: the round's totals and end -- written by the host's launch sequence)
}
// ---- the careful route's records in the same tables (msnv_measure_reads has measured them one thread a record, the blocks' sums are scanned):
// places before every record, the rd rows, run / group starts against the pileup read before (flags; their scan numbers them)
__global__ __launch_bounds__(256) void msnv_tables_from_measure(uint32_t n_rec, const uint16_t *rec_sample, const uint8_t *r_flags_in, const unsigned long long *r_key, const uint32_t *r_end, const uint32_t *r_maxc,
                                                                const RecCnt *r_cnt, const RecCnt *blk_pre, const uint32_t *r_ftile, uint32_t span_out, DpParams P, RdTables T, unsigned long long *start_flags, DpAcc *acc, uint32_t *misc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = i < n_rec;
    const RecCnt mine = valid ? r_cnt[i] : RecCnt{};
    const RecCnt pre = cnt_add(blk_pre[(valid ? i : n_rec - 1u) / PB], wave_excl_cnt(mine));
    uint8_t fl = valid ? r_flags_in[i] : 0;
    const uint32_t s = valid ? rec_sample[i] : 0u, ft = valid ? r_ftile[i] : 0u;
    const unsigned long long key = valid ? r_key[i] : 0ull;
    const bool pile = (fl & RF_PILE) != 0;
    // the pileup read before this one: a lane of the wavefront, or -- for the first one of the wavefront -- looked for in the records in front
    const unsigned long long pm = __ballot(pile), below = pm & ((1ull << lane) - 1ull);
    const int src = below ? 63 - __builtin_clzll(below) : 0;
    unsigned long long pk = __shfl(key, src); uint32_t ps = __shfl(s, src), pf = __shfl(ft, src);
    bool have_prev = below != 0ull;
    if (pile && !have_prev) {
        for (uint32_t j = i - lane; j > 0 && !have_prev;) { --j; if (r_flags_in[j] & RF_PILE) { have_prev = true; pk = r_key[j]; ps = rec_sample[j]; pf = r_ftile[j]; } }
    }
    unsigned long long sf = 0;
    if (valid) {
        uint32_t outl = 0;
        if (pile) {
            const bool run = !have_prev || ps != s || (uint32_t)(pk >> 32) != (uint32_t)(key >> 32), grp = run || pf != ft;
            if (run) fl |= RF_RUN;
            if (grp) fl |= RF_GRP;
            if (!run && pf > ft) atomicOr(&misc[MISC_SORT], 1u);                         // (a read whose first aligned base lies in an earlier tile than its predecessor's: leading deletions)
            sf = (unsigned long long)(run ? 1u : 0u) << 32 | (grp ? 1u : 0u);
            const uint32_t span = r_end[i] - ((uint32_t)key & 0x7fffffffu);
            outl = span > span_out ? 1u : 0u;
            if (r_maxc[i] >= MAXC_SAT && P.token_limit > 0) atomicOr(&acc[(size_t)s * ACC_COPIES].need_host, NEED_TOKEN | NEED_BIGC);
        }
        const uint32_t mc = r_maxc[i] < MAXC_SAT ? r_maxc[i] : MAXC_SAT;
        T.rd[i] = make_uint4((uint32_t)key, r_end[i], (uint32_t)(key >> 32), (s & 0xfffu) | outl << 12 | mc << 13);
        T.r_pre[i] = pre; T.r_flags[i] = fl; T.r_ftile[i] = ft;
        start_flags[i] = sf;
    }
}
// ---- depth at every read start, over the RECORDS (round 6: no list of the pileup reads, no scan of their run / group flags -- both come with the
// records' tables).  A record that is no pileup read is stepped over by its neighbours' walks; everything else is msnv_depth's.
__global__ __launch_bounds__(256) void msnv_depth2(uint32_t n_rec, const uint4 *rd, const uint8_t *r_flags, const unsigned long long *r_rg, const RecCnt *r_pre, const uint32_t *r_ftile,
                                                   const uint32_t *ovr, DpParams P, const uint32_t *misc_span, const uint32_t *outliers, const uint32_t *misc_nout,
                                                   uint16_t *pdepth, const uint2 *grp_pre, uint32_t in_order, uint32_t *run_first, uint32_t *run_f1, uint32_t *grp_first, uint32_t *grp_md, DpAcc *acc,
                                                   uint32_t *r_depth0, uint32_t *hot, uint32_t *hot_n) {       // (the careful route's, may be NULL: the depth of every pileup read, the reads whose sample's base string may reach the token limit)
    __shared__ uint4 s_rd[DEPTH_BACK + 256];
    __shared__ uint8_t s_fl[DEPTH_BACK + 256];
    const uint32_t blk0 = blockIdx.x * blockDim.x, i = blk0 + threadIdx.x;
    const uint32_t lds_lo = blk0 > DEPTH_BACK ? blk0 - DEPTH_BACK : 0u, lds_n = (blk0 + 256u < n_rec ? blk0 + 256u : n_rec) - lds_lo;
    for (uint32_t k = threadIdx.x; k < lds_n; k += 256u) { s_rd[k] = rd[lds_lo + k]; s_fl[k] = r_flags[lds_lo + k]; }
    __syncthreads();
    const uint8_t fl = i < n_rec ? s_fl[i - lds_lo] : 0;
    const bool valid = (fl & RF_PILE) != 0;
    uint32_t gi = 0xffffffffu, depth = 0, spill = 0;
    if (valid) {
        const uint32_t window = *misc_span;
        uint32_t n_out = *misc_nout; n_out = n_out < CAP_OUT ? n_out : CAP_OUT;
        const uint4 me4 = s_rd[i - lds_lo];
        const uint32_t p = me4.x;
        const unsigned long long me = r_rg[i];
        const uint32_t g = (uint32_t)(me >> 32) - 1u;
        gi = (uint32_t)me - 1u;
        const uint32_t my_sample = me4.w & 0xfffu;
        const bool run_start = (fl & RF_RUN) != 0;
        if (run_start) run_first[g] = i;
        if (fl & RF_GRP) grp_first[gi] = i;
        unsigned long long chars = me4.w >> 13;
        depth = 1;
        const unsigned long long pw = p;                                                    // a read is inside while start + window > p
        uint32_t j = i;                                                                     // records [j, i) have been looked at
        bool out = false, seen_prev = false; uint32_t prev_x = 0;
        while (j > lds_lo) {
            const uint32_t k = j - 1u - lds_lo;
            if (!(s_fl[k] & RF_PILE)) { --j; continue; }
            const uint4 x = s_rd[k];
            if (!seen_prev) { seen_prev = true; prev_x = x.x; }
            if (x.z != me4.z || (x.w & 0xfffu) != my_sample || (unsigned long long)x.x + window <= pw) { out = true; break; }
            if (x.y > p && !(x.w & 0x1000u)) { ++depth; chars += x.w >> 13; }
            --j;
        }
        while (!out && j > 0) {
            const uint32_t k = j - 1u;
            if (!(r_flags[k] & RF_PILE)) { --j; continue; }
            const uint4 x = rd[k];
            if (!seen_prev) { seen_prev = true; prev_x = x.x; }
            if (x.z != me4.z || (x.w & 0xfffu) != my_sample || (unsigned long long)x.x + window <= pw) { out = true; break; }
            if (x.y > p && !(x.w & 0x1000u)) { ++depth; chars += x.w >> 13; }
            --j;
        }
        for (uint32_t k = 0; k < n_out; ++k) {                                              // the round's far-reaching reads: alive here when of this run, before i, ending beyond p
            const uint32_t o = outliers[k];
            if (o < i) { const uint4 x = rd[o]; if ((x.w & 0xfffu) == my_sample && x.z == me4.z && x.y > p) { ++depth; chars += x.w >> 13; } }
        }
        // first read of the run whose end lies beyond position 1 (the first line under metaSNV's `name 1 LEN` split): a read that starts at
        // position >= 1 always qualifies, so only the reads at position 0 and the first one behind them can be it -- a handful of atomics per run
        if (me4.y > 1u && (run_start || p == 0u || (seen_prev && prev_x == 0u))) atomicMin(&run_f1[g], i);
        const RecCnt pa = r_pre[i], pb = r_pre[i + 1u];
        spill = pb.spill - pa.spill;
        const uint32_t ov = ovr ? ovr[i] : 0u;
        if ((ov & 9u) == 1u) depth = ov >> 16;                                              // (the host pre-pass's; 9: msnv_cap_reads has decided who enters, the depth is this walk's)
        else {
            if (r_depth0) r_depth0[i] = depth;
            const bool tok = P.token_limit > 0 && chars >= (unsigned long long)P.token_limit;
            if (tok && hot) hot[atomicAdd(hot_n, 1u)] = i;
            if (!(ov & 1u)) {
                uint32_t need = 0;
                if (P.max_depth > 0 && depth - 1u > (uint32_t)P.max_depth) need |= NEED_CAP;     // live.size() > max_depth before the push
                if (tok) need |= NEED_TOKEN;
                if (need) atomicOr(&acc[(size_t)my_sample * ACC_COPIES].need_host, need);
            }
            depth = depth < 0xffffu ? depth : 0xffffu;
        }
        // the depth of every piece of this read, at the piece's header slot (round 6: the emit kernels do not wait for this kernel any more --
        // the places are the ones msnv_emit_block computes: file order, or the group's own-tile / next-tile stretches of the tile order)
        const uint32_t np = pb.npiece - pa.npiece;
        if (np) {
            const uint16_t dv = (uint16_t)depth;
            if (in_order) for (uint32_t k = 0; k < np; ++k) pdepth[pa.npiece + k] = dv;
            else {
                const uint2 pf = grp_pre[gi], pe = grp_pre[gi + 1u];
                const uint32_t d_own = pa.npiece - (pa.spill - pf.y), d_next = pe.x - pe.y + pa.spill;
                for (uint32_t k = 0; k < np - spill; ++k) pdepth[d_own + k] = dv;
                for (uint32_t k = 0; k < spill; ++k) pdepth[d_next + k] = dv;
            }
        }
    }
    // depth bounds per group: [2 gi] over all its reads (every read has a piece in its first tile), [2 gi + 1] over the reads that leave
    // pieces in the tile behind.  A wavefront's reads nearly always share one group: one atomic per wavefront and bound then.
    uint32_t g_any = gi;
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(g_any, o); g_any = x < g_any ? x : g_any; }      // (a group of the wavefront, if it has a pileup read at all)
    if (g_any != 0xffffffffu) {
        if (__all(gi == g_any || !valid)) {
            uint32_t a = valid ? depth : 0u, b = (valid && spill) ? depth : 0u;
            for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(a, o), y = __shfl_xor(b, o); a = x > a ? x : a; b = y > b ? y : b; }
            if ((threadIdx.x & 63u) == 0) { atomicMax(&grp_md[2u * g_any], a); if (b) atomicMax(&grp_md[2u * g_any + 1u], b); }
        } else if (valid) { atomicMax(&grp_md[2u * gi], depth); if (spill) atomicMax(&grp_md[2u * gi + 1u], depth); }
    }
}
// ------------------------------------------------------------------------------------------ the depth cap and the token limit as kernels (round 6)
// The two sequential edits that were the host pre-pass's alone (pack.cpp: filter_and_edit's heap, apply_token_limit), for the samples whose
// records can trigger them (NEED_CAP / NEED_TOKEN, raised by msnv_depth2's bounds).
//
// mpileup -d (sam.c bam_plp_push [EXT], sample-local as pack.cpp restates it): a read that is not the first to start at its position is
// dropped when more than max_depth reads that ENTERED are alive there.  Sequential -- a dropped read is not alive for the next one -- but only
// where it can matter: msnv_depth2 has counted, for every read, the pileup reads alive at its start whether they entered or not (depth0); a
// read with depth0 - 1 <= max_depth enters whatever was dropped before it.  The others ("uncertain": a deep stack's) are taken one by one,
// by the sample's ONE wavefront: alive and entered = depth0 - 1 - (dropped reads still alive), the latter kept as a count and, per end
// position, in a ring of CAP_RING positions in LDS (a read spans at most SPAN_OUT = CAP_RING positions here; a round with far-reaching reads
// keeps the host pre-pass).  Out: the verdict per record in the host pre-pass's form, bit 3 = "the depth is not given: msnv_depth2 counts
// it" -- the careful route's second pass measures with these verdicts, so the dropped reads are out of every later count, of the
// overlapping-mate candidates (sam.c overlap_remove) and of the columns.
constexpr uint32_t CAP_RING = SPAN_OUT;
__global__ __launch_bounds__(64) void msnv_cap_reads(const uint32_t *samples, const uint32_t *rec_base, const uint4 *rd, const uint8_t *r_flags, const uint32_t *depth0, int max_depth, uint32_t *ovr, uint32_t *fail) {
    __shared__ uint32_t ring[CAP_RING];                               // dropped reads that end at position e: ring[e mod CAP_RING], for e in (cur, cur + CAP_RING]
    const uint32_t s = samples[blockIdx.x], lane = threadIdx.x;
    const uint32_t rb = rec_base[s], re = rec_base[s + 1u];
    for (uint32_t k = lane; k < CAP_RING; k += 64u) ring[k] = 0u;
    __syncthreads();
    uint32_t cur_tid = 0xffffffffu, cur = 0u, c = 0u;                 // c: dropped reads alive at `cur`
    uint32_t prev_tid = 0xffffffffu, prev_pos = 0u; bool have_prev = false;      // the pileup read before, in file order
    for (uint32_t base = rb; base < re; base += 64u) {
        const uint32_t i = base + lane;
        const bool valid = i < re;
        const uint8_t fl = valid ? r_flags[i] : (uint8_t)0;
        const uint4 x = valid ? rd[i] : make_uint4(0u, 0u, 0u, 0u);
        const bool pile = (fl & RF_PILE) != 0;
        const unsigned long long m = __ballot(pile), below = m & ((1ull << lane) - 1ull);
        const int src = below ? 63 - __builtin_clzll(below) : 0;
        uint32_t ptid = __shfl(x.z, src), ppos = __shfl(x.x, src);
        bool hp = true;
        if (!below) { ptid = prev_tid; ppos = prev_pos; hp = have_prev; }
        const bool first_at = !hp || ptid != x.z || ppos != x.x;
        const uint32_t d0 = pile ? depth0[i] : 0u;
        const bool uncertain = pile && !first_at && max_depth > 0 && d0 - 1u > (uint32_t)max_depth;
        if (m) { const int top = 63 - __builtin_clzll(m); prev_tid = __shfl(x.z, top); prev_pos = __shfl(x.x, top); have_prev = true; }
        bool dropped = false;
        unsigned long long um = __ballot(uncertain);
        while (um) {
            const int l = __builtin_ctzll(um);
            um &= um - 1ull;
            const uint32_t t_l = __shfl(x.z, l), p_l = __shfl(x.x, l), e_l = __shfl(x.y, l), d_l = __shfl(d0, l), w_l = __shfl(x.w, l);
            if (t_l != cur_tid || p_l - cur >= CAP_RING) {                            // another contig, or beyond every end the ring holds
                if (c) { for (uint32_t k = lane; k < CAP_RING; k += 64u) ring[k] = 0u; __syncthreads(); }
                cur_tid = t_l; cur = p_l; c = 0u;
            } else if (p_l > cur) {
                if (c) {
                    uint32_t gone = 0;
                    for (uint32_t q = lane; q < p_l - cur; q += 64u) { const uint32_t k = (cur + 1u + q) & (CAP_RING - 1u); gone += ring[k]; ring[k] = 0u; }
                    for (int o = 32; o > 0; o >>= 1) gone += __shfl_xor(gone, o);
                    c -= gone;
                    __syncthreads();
                }
                cur = p_l;
            }
            if (d_l - 1u - c > (uint32_t)max_depth) {                                 // pack.cpp: `live.size() > max_depth`
                if ((w_l & 0x1000u) || e_l - p_l > CAP_RING) { if (lane == 0) *fail = 1u; }      // (a far-reaching read: not this kernel's)
                else if (lane == 0) ring[e_l & (CAP_RING - 1u)] += 1u;
                ++c;
                if ((int)lane == l) dropped = true;
                __syncthreads();
            }
        }
        if (valid) ovr[i] = 1u | 8u | ((pile && !dropped) ? 2u : 0u) | ((fl & RF_COV) ? 4u : 0u);
    }
}
// snpCall's token limit (call_vC.cpp:92-111,481-483; pack.cpp: apply_token_limit states what is counted): a sample's base string is cut
// at token_limit characters, the bases behind the cut are never counted.  Which bases those are is a matter of ONE position: the elements of
// the reads alive there, in file order, each [^ mapq] base|*|<> [+n ins | -n del] [$] unless its quality is below -Q.  msnv_depth2 lists the
// read starts where the sum of the alive reads' longest elements reaches the limit (`hot`); the string can only be that long from the LAST
// read start at such a position up to the next read start (no read arrives in between: the bound only falls).  A workgroup per listed
// start: position after position, the records from the first one that can be alive here up to the start, 256 at a time: every thread finds
// its read's element at the position (the CIGAR operation that holds it: pack.cpp's cursor, from the read's start), a scan of the elements'
// lengths says where each begins, and a base whose character lies at or behind the limit gets bit 7 of its quality set -- the mark
// piece_lane reads as "below every cutoff" (every quality of such a sample's pileup reads is clamped to 127 first: msnv_token_clamp; the
// element in front of a deletion is judged by the quality of the NEXT base, which another position may be marking: bit 7 is masked out).
__global__ void msnv_token_clamp(const uint8_t *tok_sample, const uint16_t *rec_sample, const uint8_t *r_flags, uint32_t n_rec, uint8_t *raw, const unsigned long long *rec_off) {
    const uint32_t i = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (i >= n_rec || !(r_flags[i] & RF_PILE) || !tok_sample[rec_sample[i]]) return;
    const Rec r = rec_load(raw + rec_off[i], rec_off[i + 1u] - rec_off[i]);
    uint8_t *q = raw + (r.qual - raw);
    for (uint32_t j = lane; j < (uint32_t)r.l_seq; j += 64u) if (q[j] > 127u) q[j] = 127u;
}
__device__ __forceinline__ uint32_t decimal_digits_dev(uint32_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; ++d; } return d; }
__global__ __launch_bounds__(256) void msnv_token_cut(const uint32_t *hot, const uint32_t *hot_n, const uint8_t *tok_sample, const uint32_t *rec_base, const uint4 *rd, const uint8_t *r_flags,
                                                      uint8_t *raw, const unsigned long long *rec_off, const uint32_t *misc_span, DpParams P) {
    __shared__ uint32_t sh_a, sh_b, sh_lo;
    __shared__ unsigned long long w_chars[4], w_bound[4];
    const uint32_t n_hot = *hot_n, window = *misc_span, t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const unsigned long long limit = (unsigned long long)P.token_limit;
    for (uint32_t h = blockIdx.x; h < n_hot; h += gridDim.x) {
        const uint32_t i = hot[h];
        const uint4 me = rd[i];
        const uint32_t s = me.w & 0xfffu;
        if (!tok_sample[s]) continue;
        const uint32_t rb = rec_base[s], re = rec_base[s + 1u];
        __syncthreads();
        if (t == 0) {                                                                       // the next pileup read of the sample: another start at this position takes the position; else it bounds the stretch
            uint32_t j = i + 1u;
            while (j < re && !(r_flags[j] & RF_PILE)) ++j;
            uint32_t a = 1u, b = 0xffffffffu;
            if (j < re) { const uint4 y = rd[j]; if (y.z == me.z) { if (y.x == me.x) a = 0u; b = y.x; } }
            sh_a = a; sh_b = b; sh_lo = rb;
        }
        __syncthreads();
        if (!sh_a) continue;
        const uint32_t p_end = sh_b;
        // the first record that can be alive at the start: behind the last pileup read in front that lies outside the window (msnv_depth2's test)
        for (uint32_t top = i; top > rb;) {
            const uint32_t n = top - rb < 256u ? top - rb : 256u;
            uint32_t found = 0;
            if (t < n) {
                const uint32_t j = top - 1u - t;
                if (r_flags[j] & RF_PILE) { const uint4 y = rd[j]; if (y.z != me.z || (unsigned long long)y.x + window <= (unsigned long long)me.x) found = j + 1u; }
            }
            if (found) atomicMax(&sh_lo, found);
            __syncthreads();
            const bool done = sh_lo != rb;
            __syncthreads();
            if (done) break;
            top -= n;
        }
        const uint32_t lo = sh_lo;
        for (uint32_t p = me.x; p < p_end; ++p) {
            unsigned long long off = 0, bound = 0;                                          // characters of the string in front of this chunk; sum of the alive reads' longest elements
            for (uint32_t c0 = lo; c0 <= i; c0 += 256u) {
                const uint32_t j = c0 + t;
                uint32_t chars = 0, head2 = 0, maxc = 0; uint8_t *mark = nullptr;
                if (j <= i && (r_flags[j] & RF_PILE)) {
                    const uint4 y = rd[j];
                    if (y.z == me.z && y.x <= p && y.y > p) {
                        maxc = y.w >> 13;
                        const uint8_t *rp = raw + rec_off[j];
                        const Rec r = rec_load(rp, rec_off[j + 1u] - rec_off[j]);
                        long long x = r.pos, q = 0; uint32_t k = 0, tt = 0; long long l = 0; bool found = false;
                        for (; k < r.n_cigar; ++k) {
                            const uint32_t cg = ld32(r.cigar + 4ull * k);
                            tt = cg & 15u; l = cg >> 4;
                            if (cg_ref(tt) && (long long)p < x + l) { found = true; break; }
                            if (cg_ref(tt)) x += l;
                            if (cg_query(tt)) q += l;
                        }
                        if (found) {
                            const bool is_del = !cg_match(tt);
                            const long long qpos = is_del ? q : q + ((long long)p - x);
                            unsigned long long n_indel = 0;
                            if (!is_del && x + l - 1 == (long long)p && k + 1u < r.n_cigar) {
                                const uint32_t c2 = ld32(r.cigar + 4ull * (k + 1u)), t2 = c2 & 15u;
                                if (t2 == C_D || t2 == C_I) n_indel = c2 >> 4;
                                else if (t2 == C_P && k + 2u < r.n_cigar) {
                                    for (uint32_t k3 = k + 2u; k3 < r.n_cigar; ++k3) {
                                        const uint32_t c3 = ld32(r.cigar + 4ull * k3), t3 = c3 & 15u;
                                        if (t3 == C_I) n_indel += c3 >> 4;
                                        else if (t3 == C_D || t3 == C_M || t3 == C_N || t3 == C_EQ || t3 == C_X) break;
                                    }
                                }
                            }
                            uint8_t *qual = r.l_seq > 0 ? raw + (r.qual - raw) : nullptr;
                            const int qv = (qual && qpos < (long long)r.l_seq) ? (int)(qual[qpos] & 0x7fu) : 0;
                            if (!P.all_low && qv >= P.c_eff) {                                // (printed at all: bam_plcmd.c's -Q test)
                                const bool head = p == (uint32_t)r.pos, tail = p == y.y - 1u;
                                head2 = head ? 2u : 0u;
                                const unsigned long long ch = head2 + 1ull + (n_indel ? 1ull + decimal_digits_dev((uint32_t)n_indel) + n_indel : 0ull) + (tail ? 1ull : 0ull);
                                chars = (uint32_t)(ch < 0x7fffffffull ? ch : 0x7fffffffull);
                                if (!is_del && qual) mark = qual + qpos;
                            }
                        }
                    }
                }
                // where this thread's element begins: the chunk's elements in front of it
                unsigned long long incl = chars, bsum = maxc;
                for (int o = 1; o < 64; o <<= 1) { const unsigned long long v = __shfl_up(incl, o); if ((int)lane >= o) incl += v; }
                for (int o = 32; o > 0; o >>= 1) bsum += __shfl_xor(bsum, o);
                __syncthreads();
                if (lane == 63u) { w_chars[wv] = incl; w_bound[wv] = bsum; }
                __syncthreads();
                unsigned long long before = off;
                for (uint32_t w = 0; w < wv; ++w) before += w_chars[w];
                const unsigned long long begin = before + incl - chars;
                if (mark && begin + head2 >= limit) *mark = (uint8_t)(*mark | 0x80u);           // the base's own character is cut off
                off += w_chars[0] + w_chars[1] + w_chars[2] + w_chars[3];
                bound += w_bound[0] + w_bound[1] + w_bound[2] + w_bound[3];
            }
            if (bound < limit) break;                                                       // nothing arrives before p_end: the string stays below the limit from here on
        }
    }
}
__global__ void msnv_run_table2(uint32_t n_runs, const uint32_t *run_first, const uint32_t *run_f1, const uint4 *rd, DpRun *runs) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_runs) return;
    const uint4 a = rd[run_first[g]];
    DpRun o;
    o.sample = a.w & 0xfffu; o.tid = (int32_t)a.z; o.first_any = (int32_t)a.x;
    const uint32_t f = run_f1[g];
    if (f == 0xffffffffu) o.first_from1 = -1;
    else { const int32_t q = (int32_t)rd[f].x; o.first_from1 = q > 1 ? q : 1; }
    runs[g] = o;
}
__global__ void msnv_group_firsts(uint32_t n_rec, const uint8_t *r_flags, const unsigned long long *r_rg, uint32_t *run_first, uint32_t *grp_first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !(r_flags[i] & RF_PILE)) return;
    const unsigned long long me = r_rg[i];
    if (r_flags[i] & RF_RUN) run_first[(uint32_t)(me >> 32) - 1u] = i;
    if (r_flags[i] & RF_GRP) grp_first[(uint32_t)me - 1u] = i;
}
__global__ void msnv_group_pre2(uint32_t n_groups, uint32_t n_rec, const uint32_t *grp_first, const RecCnt *r_pre, uint2 *grp_pre) {
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi > n_groups) return;
    const RecCnt pf = r_pre[gi < n_groups ? grp_first[gi] : n_rec];
    grp_pre[gi] = make_uint2(pf.npiece, pf.spill);
}
__global__ void msnv_group_table2(uint32_t n_groups, uint32_t n_rec, const uint32_t *grp_first, const RecCnt *r_pre, const uint4 *rd, const uint32_t *r_ftile, const uint32_t *grp_md, uint2 *grp_pre, DevGroupRec *out) {
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi > n_groups) return;
    const uint32_t f = gi < n_groups ? grp_first[gi] : n_rec;
    const RecCnt pf = r_pre[f];
    if (grp_pre) grp_pre[gi] = make_uint2(pf.npiece, pf.spill);      // (NULL: msnv_group_pre2 has written them)
    if (gi == n_groups) return;
    const uint32_t e = gi + 1u < n_groups ? grp_first[gi + 1u] : n_rec;
    const RecCnt pe = r_pre[e];
    const uint4 a = rd[f];
    DevGroupRec o;
    o.sample = a.w & 0xfffu; o.tid = (int32_t)a.z; o.tile = r_ftile[f];
    o.a = pf.npiece; o.b = pe.npiece - (pe.spill - pf.spill); o.end = pe.npiece; o.md_own = grp_md[2u * gi]; o.md_next = grp_md[2u * gi + 1u];
    out[gi] = o;
}
// per sample: where its records' pieces / seq bytes / intervals start, the first pileup read -- and where its columns lie in the round's buffer
// (round 6: the layout is the device's; the host sized the buffer by the round's totals and learns the shares with the other small results)
struct DpSampleSum2 { unsigned long long sbase0, first_key, beyond_key, seq_off; uint32_t pbase0, ibase0, first_end, pad; };
__global__ void msnv_sample_layout(const uint32_t *rec_base, uint32_t n_samples, const RecCnt *r_pre, const DpAcc *acc, const uint4 *rd, uint8_t *r_seq, uint8_t *r_qual, const uint8_t *cut_marks,
                                   DpSampleSum2 *out, unsigned long long *sbase0, DpSampleDst *dst, unsigned long long *piece_bytes) {
    const uint32_t s = threadIdx.x;                                  // ONE workgroup: the shares are a running sum over the samples (<= 2048 of them a round)
    __shared__ unsigned long long sh[2049];
    for (uint32_t k = s; k <= n_samples; k += blockDim.x) sh[k] = r_pre[rec_base[k]].seqb;
    __syncthreads();
    if (s == 0) {
        unsigned long long o = 0;
        for (uint32_t k = 0; k < n_samples; ++k) { const unsigned long long pb = sh[k + 1] - sh[k]; sh[k] = o; o += (pb + 32ull + 15ull) & ~15ull; }
        sh[n_samples] = o;
    }
    __syncthreads();
    for (uint32_t k = s; k <= n_samples; k += blockDim.x) {
        const RecCnt pre = r_pre[rec_base[k]];
        DpSampleSum2 o{};
        o.sbase0 = pre.seqb; o.pbase0 = pre.npiece; o.ibase0 = pre.niv; o.seq_off = sh[k];
        sbase0[k] = pre.seqb;
        if (k < n_samples) {
            const DpAcc a = acc[(size_t)k * ACC_COPIES];              // (folded: msnv_acc_fold)
            if (a.first_pile != ~0ull) { const uint4 x = rd[a.first_pile]; o.first_key = (unsigned long long)x.z << 32 | x.x; o.first_end = x.y; }
            if (a.beyond != ~0ull) { const uint4 x = rd[a.beyond]; o.beyond_key = (unsigned long long)x.z << 32 | x.x; }
            dst[k] = DpSampleDst{r_seq + sh[k], r_qual + sh[k] / 4, pre.npiece, cut_marks ? cut_marks[k] : 0u, 0u};
            piece_bytes[k] = r_pre[rec_base[k + 1]].seqb - pre.seqb;
        }
        out[k] = o;
    }
}

// ------------------------------------------------------------------------------------------ overlapping mates
// `samtools mpileup` without -x lets htslib's pileup engine edit the qualities of proper-pair mates that overlap on the reference before
// the -Q cutoff sees them (sam.c overlap_push / tweak_overlap_quality [EXT]; pack.cpp: filter_and_edit restates the engine, read after read,
// with a hash of waiting mates by read name).  The entries of different names never interact, so the walk is independent per NAME: the
// candidates of a round are sorted by (sample, hash of the name) -- stable, so file order survives inside a group -- and one thread runs
// the engine's state machine over each group: a read finds the waiting mate of its name (alive: same contig, end beyond this start), the
// pair is edited in place in the round buffer and the entry leaves; else the read waits if its mate is still to come.  Groups are two
// reads almost always; names are compared byte for byte inside a group (hash collisions make a group bigger, never wrong).
constexpr int OVL_SLOTS = 8;
__global__ void msnv_ovl_list(const uint8_t *r_flags, const uint32_t *orank, uint32_t n_rec, const uint8_t *raw, const unsigned long long *rec_off, const uint16_t *rec_sample,
                              const uint8_t *skip_sample, unsigned long long *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !(r_flags[i] & RF_OVL) || skip_sample[rec_sample[i]]) return;
    const uint8_t *p = raw + rec_off[i];
    const uint32_t l_name = p[12];
    unsigned long long h = 1469598103934665603ull;                // FNV-1a over the name
    for (uint32_t k = 0; k < l_name; ++k) { h ^= p[36 + k]; h *= 1099511628211ull; }
    const uint32_t w = orank[i];
    keys[w] = (unsigned long long)rec_sample[i] << 53 | (h >> 11);
    vals[w] = i;
}
__global__ void msnv_ovl_mark(const uint8_t *r_flags, uint32_t n_rec, const uint16_t *rec_sample, const uint8_t *skip_sample, uint32_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    flag[i] = (i < n_rec && (r_flags[i] & RF_OVL) && !skip_sample[rec_sample[i]]) ? 1u : 0u;
}
__global__ void msnv_ovl_group_starts(const uint32_t *flag, const uint32_t *gid_incl, uint32_t n, uint32_t *starts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) starts[gid_incl[i] - 1u] = i;
}
// groups of more than OVL_SLOTS members could overflow the waiting slots: their samples take the host pre-pass (decided BEFORE anything is edited)
__global__ void msnv_ovl_check(const uint32_t *starts, uint32_t n_groups, uint32_t n, const uint32_t *svals, const uint16_t *rec_sample, DpAcc *acc) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t lo = starts[g], hi = g + 1 < n_groups ? starts[g + 1] : n;
    if (hi - lo > (uint32_t)OVL_SLOTS) atomicOr(&acc[(size_t)rec_sample[svals[lo]] * ACC_COPIES].need_host, NEED_OVL);
}
struct MatchCur {                                               // the M/=/X bases of one alignment in reference order (pack.cpp: MatchCursor)
    const uint8_t *cigar; uint32_t n_cigar, k; long long op_ref, op_q, ref, q;
    __device__ bool seek(const long long target) {
        for (; k < n_cigar; ++k) {
            const uint32_t c = ld32(cigar + 4ull * k), t = c & 15u; const long long l = c >> 4;
            if (cg_match(t)) {
                if (target < op_ref + l) { ref = target > op_ref ? target : op_ref; q = op_q + (ref - op_ref); return true; }
                op_ref += l; op_q += l;
            } else {
                if (t == C_D || t == C_N) op_ref += l;
                if (t == C_I || t == C_S) op_q += l;
            }
        }
        return false;
    }
};
__device__ void tweak_pair(uint8_t *pa, const Rec &a, uint8_t *pb, const Rec &b) {          // pack.cpp: tweak_overlapping_mates (qualities edited in the round buffer)
    if (a.l_seq == 0 || b.l_seq == 0) return;
    MatchCur ca{a.cigar, a.n_cigar, 0u, a.pos, 0, -1, -1}, cb{b.cigar, b.n_cigar, 0u, b.pos, 0, -1, -1};
    uint8_t *qa = pa + (a.qual - (const uint8_t *)pa), *qb = pb + (b.qual - (const uint8_t *)pb);
    long long t = b.pos;
    while (ca.seek(t) && cb.seek(ca.ref)) {
        t = cb.ref + 1;
        if (ca.ref != cb.ref) continue;
        if (ca.q >= a.l_seq || cb.q >= b.l_seq) return;
        const uint32_t ba = (a.seq[ca.q >> 1] >> ((~ca.q & 1) << 2)) & 0xfu, bb = (b.seq[cb.q >> 1] >> ((~cb.q & 1) << 2)) & 0xfu;
        const uint32_t x = qa[ca.q], y = qb[cb.q];
        if (ba == bb) { const uint32_t sum = x + y; qa[ca.q] = (uint8_t)(sum > 200u ? 200u : sum); qb[cb.q] = 0; }
        else if (x >= y) { qa[ca.q] = (uint8_t)(0.8 * (double)x); qb[cb.q] = 0; }
        else { qb[cb.q] = (uint8_t)(0.8 * (double)y); qa[ca.q] = 0; }
    }
}
__global__ void msnv_ovl_groups(const uint32_t *starts, uint32_t n_groups, uint32_t n, const uint32_t *svals, uint8_t *raw, const unsigned long long *rec_off,
                                const uint4 *rd, const uint16_t *rec_sample, const uint8_t *skip_sample) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t lo = starts[g], hi = g + 1 < n_groups ? starts[g + 1] : n;
    if (hi - lo < 2u || hi - lo > (uint32_t)OVL_SLOTS) return;    // a lone read waits for nobody who comes; oversized groups went to the host
    if (skip_sample[rec_sample[svals[lo]]]) return;               // this sample's edits ran in the host pre-pass
    uint32_t wait[OVL_SLOTS]; int n_wait = 0;
    for (uint32_t m = lo; m < hi; ++m) {
        const uint32_t i = svals[m];
        uint8_t *p = raw + rec_off[i];
        const Rec r = rec_load(p, ~0ull);
        int found = -1;
        for (int w = 0; w < n_wait && found < 0; ++w) {            // the waiting mate of this NAME
            const uint8_t *q = raw + rec_off[wait[w]];
            if (q[12] != r.l_name) continue;
            bool same = true;
            for (uint32_t k = 0; k < r.l_name && same; ++k) same = q[36 + k] == p[36 + k];
            if (same) found = w;
        }
        if (found >= 0) {
            const uint32_t j = wait[found];
            uint8_t *q = raw + rec_off[j];
            const Rec a = rec_load(q, ~0ull);
            for (int w = found; w + 1 < n_wait; ++w) wait[w] = wait[w + 1];        // the entry leaves either way (stale: erased; alive: edited and erased)
            --n_wait;
            if (a.tid == r.tid && (long long)rd[j].y > (long long)r.pos) { tweak_pair(q, a, p, r); continue; }
        }
        if (r.mpos >= r.pos || ((r.flag & 1u) && r.mpos == -1)) { if (n_wait < OVL_SLOTS) wait[n_wait++] = i; }
    }
}

// ------------------------------------------------------------------------------------------ bases and quality flags
// FOUR lanes per piece, 32 bases per lane (round 4; the first form took 16 lanes of 8 bases: 6.4 ms on the benchmark shape against 2.x here):
// three 8-byte loads of BAM nibbles, four of phred bytes; 16 bytes of the seq column and 32 flags out.
__device__ __forceinline__ uint64_t nib_swap64(uint64_t b) { return ((b >> 4) & 0x0f0f0f0f0f0f0f0full) | ((b & 0x0f0f0f0f0f0f0f0full) << 4); }
// bit t = byte t of q is a quality below c (1 <= c <= 127; bytes of 128 and more -- "not stored", clamped to 127 by the host stage -- are not)
__device__ __forceinline__ uint32_t low_flags8(uint64_t q, uint32_t c) {
    const uint64_t y = (q | 0x8080808080808080ull) - 0x0101010101010101ull * c;            // bit 7 of a byte: (q & 0x7f) >= c; no borrow between bytes
    const uint64_t lt = ~(q | y) & 0x8080808080808080ull;
    return (uint32_t)(((lt >> 7) * 0x0102040810204080ull) >> 56);
}

// ------------------------------------------------------------------------------------------ headers, intervals, bases: one block of records per workgroup
// msnv_emit_block (round 5; rounds 4's msnv_emit_headers + msnv_emit_pieces went to every record twice with a thread's worth of scattered
// loads each): a workgroup takes a block of PB records -- consecutive in the round buffer --, stages their bytes in LDS with coalesced
// 16-byte loads (every byte of the records is read from HBM once), then
//   one thread per record: header and CIGAR from LDS -> qaCompute's intervals (qaCompute.cpp:530-552), the piece headers at their places
//     in tile order, and a descriptor of every piece in LDS;
//   four lanes per piece, 32 bases a lane: BAM nibble swap, '=' -> reference code, the -Q flag of every base from the phred bytes, mismatch
//     sample of every 16th piece -- from LDS, out to the sample's columns.
// A block whose records do not fit the window (long reads), that cuts more pieces than the list holds, or that holds a record whose
// CIGAR may live in the CG field takes the direct route: a thread per record does the same from global memory, piece after piece.
//
// Tile order without a sort.  The headers of a sample must end up grouped by (contig, tile), read order inside a tile (pack.cpp's stable
// sort); in file order only the pieces a read leaves in the tile BEHIND its first one are out of place.  Reads sorted by start whose
// pieces lie in their first tile and at most the next one (msnv_measure_reads checks it; else `in_order`: file order here, rocPRIM sort
// afterwards) fall into groups of consecutive reads with the same first tile, and the sorted order is, group after group: the group's
// pieces in its own tile, then the ones it leaves in the next tile (which thereby precede the next group's own pieces -- same tile -- in
// read order).  With npiece / spill = pieces / next-tile pieces of all earlier reads and f, e = first read of this / the next group:
//   a piece in the read's first tile goes to  npiece(i) - (spill(i) - spill(f)) + its index among the read's such pieces,
//   a piece in the tile behind goes to        npiece(e) - spill(e) + spill(i)   + its index among those.
constexpr uint32_t EW_BYTES = 20480;                              // LDS window of a block's records (320 bytes a record)
struct LdsSrc {                                                   // unaligned little-endian loads from the LDS window (aligned words + funnel shift: gfx9 has no unaligned ds_read)
    const uint32_t *w;
    __device__ __forceinline__ uint32_t ld32(unsigned long long o) const { const uint32_t a = (uint32_t)o; return __builtin_amdgcn_alignbyte(w[(a >> 2) + 1], w[a >> 2], a & 3u); }
    __device__ __forceinline__ uint64_t ld64(unsigned long long o) const {
        const uint32_t a = (uint32_t)o, w0 = w[a >> 2], w1 = w[(a >> 2) + 1], w2 = w[(a >> 2) + 2];
        return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, a & 3u) | (uint64_t)__builtin_amdgcn_alignbyte(w2, w1, a & 3u) << 32;
    }
};
struct GlbSrc {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t ld32(unsigned long long o) const { return msnv::ld32(p + o); }
    __device__ __forceinline__ uint64_t ld64(unsigned long long o) const { return msnv::ld64(p + o); }
};
// One lane's 32 bases of a piece: nibbles (low first) in o0 / o1, "quality below -Q" flags in bits, mismatches against the reference in mm
// when the piece is one of the sampled ones.  j0 = 32 * sub; st / have as in the caller.
// pad_in_tile: how many of the (up to three) alignment nibbles behind the piece's last base still lie in the piece's tile: those read as the
// reference the pileup kernel compares them with (N where the FASTA has nothing), the ones beyond the tile as N -- what finalize's
// msnv_fill_padding wrote in a pass of its own over every piece (0.25 ms on the benchmark shape) until round 6.
template <class Src>
__device__ __forceinline__ void piece_lane(const Src &src, unsigned long long seq_o, unsigned long long qual_o, uint32_t q0_piece, uint32_t j0, uint32_t have, unsigned long long ref_nib,
                                           uint32_t ref_left, const uint32_t *pref4, const DpParams &P, uint32_t cut_marks, bool sample_this, uint32_t pad_in_tile,
                                           uint64_t &o0, uint64_t &o1, uint32_t &bits, uint32_t &mm) {
    const bool pad_low = P.c_eff > 0 || P.all_low;                                          // padding: base N, quality byte 0 (pack.cpp: pack_sample; finalize.cpp: pack_lowq)
    o0 = ~0ull; o1 = ~0ull; bits = pad_low ? 0xffffffffu : 0u; mm = 0;
    if (!have) return;
    const bool noseq = q0_piece == 0xffffffffu;
    const uint32_t q0 = noseq ? 0u : q0_piece + j0;
    if (!noseq) {
        // BAM packs base 2i in the HIGH nibble of byte i; the kernels want base j of the piece in nibble j, low first
        const unsigned long long sp = seq_o + (q0 >> 1);
        const uint64_t s0 = nib_swap64(src.ld64(sp)), s1 = nib_swap64(src.ld64(sp + 8)), s2 = nib_swap64(src.ld64(sp + 16));
        if (q0 & 1u) { o0 = s0 >> 4 | s1 << 60; o1 = s1 >> 4 | s2 << 60; } else { o0 = s0; o1 = s1; }
    }
    if (have < 16u) { o0 |= ~0ull << (4u * have); o1 = ~0ull; } else if (have < 32u) o1 |= ~0ull << (4u * (have - 16u));
    const uint32_t left = ref_left > j0 ? ref_left - j0 : 0u;                               // FASTA characters from the lane's first position
    const uint64_t z0 = (o0 - 0x1111111111111111ull) & ~o0 & 0x8888888888888888ull, z1 = (o1 - 0x1111111111111111ull) & ~o1 & 0x8888888888888888ull;
    const uint32_t n_pad = (have & 3u) ? (4u - (have & 3u) < pad_in_tile ? 4u - (have & 3u) : pad_in_tile) : 0u;      // (have & 3: this lane holds the piece's last base)
    if ((z0 | z1) || sample_this || n_pad) {
        uint64_t r0 = ~0ull, r1 = ~0ull;                                                    // reference codes of the lane's positions (N where the FASTA has nothing)
        if (left) {
            const unsigned long long nb = ref_nib + j0;
            const uint32_t *w = pref4 + (nb >> 3);
            const uint64_t a = (uint64_t)w[0] | (uint64_t)w[1] << 32, b = (uint64_t)w[2] | (uint64_t)w[3] << 32, c = (uint64_t)w[4];
            const uint32_t sh = 4u * (uint32_t)(nb & 7u);
            r0 = sh ? (a >> sh | b << (64u - sh)) : a;
            r1 = sh ? (b >> sh | c << (64u - sh)) : b;
            if (left < 16u) { r0 |= ~0ull << (4u * left); r1 = ~0ull; } else if (left < 32u) r1 |= ~0ull << (4u * (left - 16u));
        }
        // '=' (code 0) always counts as a match (bam_plcmd.c pileup_seq [EXT]): ship the reference code, N when that is unknown or '=' itself
        if (z0 | z1) {
            for (uint32_t t = 0; t < have; ++t) {
                uint64_t &o = t < 16u ? o0 : o1; const uint64_t r = t < 16u ? r0 : r1; const uint32_t k = 4u * (t & 15u);
                if (((o >> k) & 0xfull) == 0ull) { uint64_t code = (r >> k) & 0xfull; if (code == 0ull) code = 15ull; o |= code << k; }
            }
        }
        if (sample_this) {
            const uint32_t cmp = left < have ? left : have;
            uint64_t x0 = o0 ^ r0, x1 = o1 ^ r1;
            x0 = (x0 | x0 >> 1 | x0 >> 2 | x0 >> 3) & 0x1111111111111111ull; x1 = (x1 | x1 >> 1 | x1 >> 2 | x1 >> 3) & 0x1111111111111111ull;
            if (cmp < 16u) { x0 &= (1ull << (4u * cmp)) - 1ull; x1 = 0ull; } else if (cmp < 32u) x1 &= (1ull << (4u * (cmp - 16u))) - 1ull;
            mm = (uint32_t)(__builtin_popcountll(x0) + __builtin_popcountll(x1));
        }
        if (n_pad) {                                                                        // nibbles have .. have + n_pad - 1 (all in one of the two words: have + n_pad <= a multiple of 4)
            const uint64_t m = ((1ull << (4u * n_pad)) - 1ull) << (4u * (have & 15u));
            if (have < 16u) o0 = (o0 & ~m) | (r0 & m); else o1 = (o1 & ~m) | (r1 & m);
        }
    }
    uint32_t low = 0;
    if (P.all_low) low = 0xffffffffu;
    else if (!noseq && (P.c_eff > 0 || cut_marks)) {
        const unsigned long long qp = qual_o + q0;
        const uint64_t qa = src.ld64(qp), qb = src.ld64(qp + 8), qc = src.ld64(qp + 16), qd = src.ld64(qp + 24);
        if (P.c_eff > 0) low = low_flags8(qa, (uint32_t)P.c_eff) | low_flags8(qb, (uint32_t)P.c_eff) << 8 | low_flags8(qc, (uint32_t)P.c_eff) << 16 | low_flags8(qd, (uint32_t)P.c_eff) << 24;
        if (cut_marks) {                                                                    // bit 7: behind snpCall's token limit, below every cutoff (pack.cpp: QUAL_CUT = 0xfe, msnv_token_cut: quality | 0x80;
            const uint64_t q4[4] = {qa, qb, qc, qd};                                        // every other quality of such a sample's pileup reads has been clamped to 127)
            for (uint32_t t = 0; t < 32u; ++t) if ((q4[t >> 3] >> (8u * (t & 7u))) & 0x80ull) low |= 1u << t;
        }
    }
    // (no SEQ: quality 0 -- shipped only when the cutoff is 0, where it is not below it)
    bits = have < 32u ? ((bits & (0xffffffffu << have)) | (low & ((1u << have) - 1u))) : low;
}
struct EmitArgs {
    const uint8_t *raw; const unsigned long long *rec_off; const uint16_t *rec_sample; uint32_t n_rec; const DpContig *ctg; const uint8_t *r_flags;
    const RecCnt *r_pre; const unsigned long long *samp_sbase0, *rg; const uint2 *grp_pre; uint32_t in_order;      // r_pre: places before every record (entry n_rec: totals); rg: run << 32 | group of a pileup RECORD
    ReadHdr *hdr; int32_t *ptid, *pend; int32_t *cov_tid, *cov_beg, *cov_end; uint32_t noseq_counts;
    const uint32_t *pref4; DpParams P; const DpSampleDst *dst; DpAcc *acc;
    uint32_t force_slow;                                           // MSNV_EMIT=slow (tests): every block takes msnv_emit_block_slow
    uint32_t *slow;                                                // [0] number of listed blocks, [1 ..] the blocks msnv_emit_block left to msnv_emit_block_slow
};
// One record by its four lanes (sub = 0 .. 3): every lane reads the header and walks the CIGAR (LDS: cheap), lane 0 writes the intervals
// and the piece headers, and lane `sub` moves bases 32 sub .. 32 sub + 31 of every piece (a piece holds at most SEG_MAX = 128 bases).
// Where a lane's share of a piece goes.  GlbOut: straight into the sample's columns (byte-granular stores, the nibbles shared with a
// neighbour OR-ed in atomically: put_piece_lane).  LdsOut: OR-ed into a zeroed image of the block's stretch of the columns in LDS -- five
// words of bases and two of flags per lane, no branches --, which the workgroup then writes out with whole 16-byte stores
// (msnv_emit_block; the records of a block are consecutive in their sample's columns).
struct GlbOut {
    static constexpr bool kLds = false;
    __device__ __forceinline__ void put(const DpSampleDst &d, uint32_t so, uint32_t sub, uint32_t sb, uint32_t st, uint64_t o0, uint64_t o1, uint32_t bits, uint32_t prev_last) const {
        if (st) put_piece_lane(d.seq, d.qual, so, sub, sb, st, o0, o1, bits, prev_last);
    }
};
struct LdsOut {
    static constexpr bool kLds = true;
    uint32_t *seq_w, *flag_w; uint32_t a16;                      // images of the seq / flag columns from byte a16 of the sample's seq column (a multiple of 16)
    __device__ __forceinline__ void put(const DpSampleDst &, uint32_t so, uint32_t sub, uint32_t, uint32_t st, uint64_t o0, uint64_t o1, uint32_t bits, uint32_t) const {
        if (!st) return;
        // bases: st / 2 bytes from byte L of the image; what lies beyond them in the registers must not reach the neighbour's bytes
        const uint32_t nb = st >> 1, L = so - a16 + 16u * sub, sh = 8u * (L & 3u);
        if (nb < 8u) { o0 &= (1ull << (8u * nb)) - 1ull; o1 = 0ull; } else if (nb < 16u) o1 &= (1ull << (8u * (nb - 8u))) - 1ull;
        const uint64_t l = o0 << sh, h = o1 << sh | (sh ? o0 >> (64u - sh) : 0ull);
        uint32_t *q = seq_w + (L >> 2);
        atomicOr(q, (uint32_t)l);
        atomicOr(q + 1, (uint32_t)(l >> 32));
        atomicOr(q + 2, (uint32_t)h);
        atomicOr(q + 3, (uint32_t)(h >> 32));
        if (sh) atomicOr(q + 4, (uint32_t)(o1 >> (64u - sh)));
        // flags: bit index = nibble index of the seq column
        const uint32_t fb = 2u * (so - a16) + 32u * sub, v = st < 32u ? bits & ((1u << st) - 1u) : bits;
        const uint64_t fv = (uint64_t)v << (fb & 31u);
        atomicOr(flag_w + (fb >> 5), (uint32_t)fv);
        atomicOr(flag_w + (fb >> 5) + 1, (uint32_t)(fv >> 32));
    }
};
template <class Src, class Out>
__device__ __forceinline__ void emit_record(const EmitArgs &A, const Src &src, const Out &out, unsigned long long rec_o, const RecCnt me, uint32_t sub, uint8_t f, uint32_t s, uint16_t depth, uint32_t rec_index) {
    if (!(f & (RF_PILE | RF_COV))) return;
    const int32_t tid = (int32_t)src.ld32(rec_o + 4), pos = (int32_t)src.ld32(rec_o + 8);
    const uint32_t w3 = src.ld32(rec_o + 12), fn = src.ld32(rec_o + 16);
    const int32_t l_seq = (int32_t)src.ld32(rec_o + 20);
    uint32_t n_cigar = fn & 0xffffu; const uint32_t l_name = w3 & 0xffu, mapq = (w3 >> 8) & 0xffu;
    unsigned long long cig_o = rec_o + 36 + l_name;
    const unsigned long long seq_o = cig_o + 4ull * n_cigar, qual_o = seq_o + ((unsigned long long)(uint32_t)l_seq + 1) / 2;
    if (Src::kGlobal) {                                                                     // (the direct route honours a CIGAR that lives in the CG field: rec_load)
        const Rec r = rec_load(src.base() + rec_o, ~0ull);
        cig_o = (unsigned long long)(r.cigar - src.base()); n_cigar = r.n_cigar;
    }
    // (everything the record needs from global memory is asked for here, in one go: a workgroup's time is the depth of its load chain)
    const DpContig c = A.ctg[tid];
    const DpSampleDst d = A.dst[s];
    const unsigned long long sbase0 = A.samp_sbase0[s];
    uint2 pf = make_uint2(0u, 0u), pe = make_uint2(0u, 0u);
    if ((f & RF_PILE) && !A.in_order) {
        const uint32_t gi = (uint32_t)A.rg[rec_index] - 1u;
        pf = A.grp_pre[gi]; pe = A.grp_pre[gi + 1u];
    }
    // ONE walk over the CIGAR for both tools: qaCompute's intervals (lane 0; qaCompute.cpp:530-552: every op behind a leading clip moves the
    // cursor, an M op adds {+1 at the cursor, -1 behind it}) and mpileup's aligned blocks cut into pieces
    const bool noseq = l_seq == 0;
    const bool cov = (f & RF_COV) && sub == 0, pile = (f & RF_PILE) && !(noseq && !A.noseq_counts);
    if (!cov && !pile) return;
    uint32_t w = me.npiece;                                                                   // file order
    uint32_t d_own = w, d_next = w;                                                           // tile order: next header slot in the read's first tile / the tile behind
    uint32_t ftile = 0; bool have_ftile = false;
    if (!A.in_order) {
        d_own = me.npiece - (me.spill - pf.y);
        d_next = pe.x - pe.y + me.spill;
    }
    uint32_t so = (uint32_t)(me.seqb - sbase0);
    long long rp = pos; uint32_t q = 0;                                                       // (the tile arithmetic below is msnv_measure_reads' to the letter: the two must cut the same pieces)
    const uint32_t j0 = 32u * sub;
    const long long L = c.len;
    long long pp = (long long)pos + 1;
    uint32_t wiv = me.niv, k0 = 0;
    if (cov && n_cigar > 0) { const uint32_t t = src.ld32(cig_o) & 15u; if (t == C_S || t == C_H) k0 = 1; }
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t cg = src.ld32(cig_o + 4ull * k), t = cg & 15u, l = cg >> 4;
        if (cov && k >= k0) {
            if (t == C_M) {
                if (pp >= L) { if (L >= 1) { A.cov_tid[wiv] = tid; A.cov_beg[wiv] = (int32_t)L; A.cov_end[wiv] = (int32_t)(L - 1); ++wiv; } }
                else if (pp < L - 1 && l > 0u) { A.cov_tid[wiv] = tid; A.cov_beg[wiv] = (int32_t)pp; A.cov_end[wiv] = (int32_t)(pp + l); ++wiv; }      // (the kept ones only: msnv_measure_reads / measure_one counts the same)
            }
            pp += l;
        }
        if (cg_match(t)) {
            if (pile) for (uint32_t off = 0, n = 0; off < l; off += n) {
                const long long gl = rp + off;
                const uint32_t g = (uint32_t)gl;
                const uint32_t to_tile = TILE - (uint32_t)(gl % TILE);
                n = SEG_MAX < l - off ? SEG_MAX : l - off;
                n = n < to_tile ? n : to_tile;
                const uint32_t tl = (uint32_t)(gl / TILE);
                if (!have_ftile) { ftile = tl; have_ftile = true; }
                const uint32_t dst = A.in_order ? w : (tl == ftile ? d_own++ : d_next++);
                if (sub == 0) {
                    ReadHdr h;
                    h.gpos = g; h.seqoff = so; h.cig = n; h.meta = META_PILEUP_OK | mapq << 16;
                    A.hdr[dst] = h; A.ptid[dst] = tid; A.pend[dst] = (int32_t)(g + n);
                }
                // ---- this lane's 32 bases of the piece
                unsigned long long ref_nib; uint32_t ref_left;
                const long long left = c.seq_len - gl;
                if (c.seq_len >= 0 && gl >= 0 && left > 0) { ref_nib = c.pref_off + (unsigned long long)gl; ref_left = (uint32_t)(left < 0xffffffffll ? left : 0xffffffffll); }
                else { ref_nib = c.seq_len >= 0 ? ~1ull : ~0ull; ref_left = 0; }              // ~1: a FASTA record exists but holds nothing here (sampled, nothing to compare)
                const uint32_t sb = stored_bytes(n);
                const uint32_t st = 2u * sb > j0 ? (2u * sb - j0 < 32u ? 2u * sb - j0 : 32u) : 0u;    // stored nibbles of this lane (a multiple of 4)
                const uint32_t have = n > j0 ? (n - j0 < 32u ? n - j0 : 32u) : 0u;                     // ... of which real bases
                const bool sample_this = ref_nib != ~0ull && ((w - (uint32_t)d.pbase0) & 15u) == 0u;   // one piece in 16: how noisy are these reads?
                uint64_t o0, o1; uint32_t bits, mm;
                piece_lane(src, seq_o, qual_o, noseq ? 0xffffffffu : q + off, j0, have, ref_nib, ref_left, A.pref4, A.P, d.cut_marks, sample_this && have, to_tile - n < 3u ? to_tile - n : 3u,
                           o0, o1, bits, mm);      // (no SEQ: the bases are N of quality 0)
                const uint32_t prev_last = Out::kLds ? 0u : __shfl_up(bits >> 28, 1);           // the last four flags of lane sub - 1 of the same piece (sub > 0, that lane is full)
                out.put(d, so, sub, sb, st, o0, o1, bits, prev_last);
                // mismatch sample: sum over the 4 lanes of a piece, one atomic per sampled piece
                mm += __shfl_down(mm, 2, 4); mm += __shfl_down(mm, 1, 4);
                if (sub == 0 && sample_this) {
                    DpAcc &a = A.acc[(size_t)s * ACC_COPIES + (blockIdx.x % ACC_COPIES)];
                    atomicAdd(&a.mm_bases, (unsigned long long)n);
                    if (mm) atomicAdd(&a.mm, (unsigned long long)mm);
                }
                ++w; so += sb;
            }
            rp += l; q += l;
        } else {
            if (cg_ref(t)) rp += l;
            if (cg_query(t)) q += l;
        }
    }
}
struct LdsSrcK : LdsSrc { static constexpr bool kGlobal = false; __device__ const uint8_t *base() const { return nullptr; } };
struct GlbSrcK : GlbSrc { static constexpr bool kGlobal = true; __device__ const uint8_t *base() const { return p; } };

constexpr uint32_t EO_BYTES = 6144;                               // bytes of the seq column a block's image holds (its flags: a quarter of that); with the window and the descriptors 31.4 KB: five workgroups per CU
// Round 6: the block's work in two phases.  A: ONE lane per record (the block's first wavefront) reads the header and walks the CIGAR in LDS,
// writes qaCompute's intervals and the piece headers to their places and leaves a 32-byte DESCRIPTOR per piece in LDS -- a record's first piece
// in the record's slot, every further one (an indel, a clip behind aligned bases, a tile boundary: one read in sixteen) in a slot behind the
// 64.  B: the whole workgroup moves the pieces, four lanes each, slot after slot -- 64 pieces a step, so the handful of further pieces cost one
// more step of ONE wavefront, where round 5's form (every record's four lanes walking its CIGAR with the piece body inside the loop) made
// three wavefronts in four run the body twice for one lane's sake (a quarter of the kernel's vector instructions) and walked every CIGAR
// four times.  Blocks that do not fit this form -- records longer than the window, two samples in one block, a CIGAR in the CG field, more
// further pieces than slots -- are listed and taken by msnv_emit_block_slow behind this kernel.
struct PieceDesc { uint32_t seq_o, qual_o, q0, so, ref_lo, ref_hi, ref_left, nf; };     // window offsets of the record's SEQ / QUAL, first base of the piece in the read (~0: no SEQ), byte of the seq
                                                                                       // column, reference nibble index (64 bit) + FASTA characters from there, n | sampled << 8 | padding nibbles inside the tile << 9
constexpr uint32_t EQ_CAP = 32;                                   // further pieces a block of the quick form holds
__device__ __forceinline__ void emit_walk(const EmitArgs &A, const LdsSrcK &src, unsigned long long rec_o, const RecCnt me, uint8_t f, uint16_t depth, const DpSampleDst &d, unsigned long long sbase0,
                                          const DpContig &c, const uint2 pf, const uint2 pe, PieceDesc *first_slot, PieceDesc *more_slots) {
    PieceDesc none{}; none.nf = 0u;
    *first_slot = none;
    if (!(f & (RF_PILE | RF_COV))) return;
    const int32_t tid = (int32_t)src.ld32(rec_o + 4), pos = (int32_t)src.ld32(rec_o + 8);
    const uint32_t w3 = src.ld32(rec_o + 12), fn = src.ld32(rec_o + 16);
    const int32_t l_seq = (int32_t)src.ld32(rec_o + 20);
    const uint32_t n_cigar = fn & 0xffffu, l_name = w3 & 0xffu, mapq = (w3 >> 8) & 0xffu;
    const unsigned long long cig_o = rec_o + 36 + l_name;
    const unsigned long long seq_o = cig_o + 4ull * n_cigar, qual_o = seq_o + ((unsigned long long)(uint32_t)l_seq + 1) / 2;
    const bool noseq = l_seq == 0;
    const bool cov = (f & RF_COV) != 0, pile = (f & RF_PILE) && !(noseq && !A.noseq_counts);
    if (!cov && !pile) return;
    uint32_t w = me.npiece;                                                                   // file order
    uint32_t d_own = w, d_next = w;                                                           // tile order: next header slot in the read's first tile / the tile behind
    uint32_t ftile = 0; bool have_ftile = false;
    if (!A.in_order) {
        d_own = me.npiece - (me.spill - pf.y);
        d_next = pe.x - pe.y + me.spill;
    }
    uint32_t so = (uint32_t)(me.seqb - sbase0);
    long long rp = pos; uint32_t q = 0;                                                       // (the tile arithmetic below is msnv_measure_reads' to the letter: the two must cut the same pieces)
    const long long L = c.len;
    long long pp = (long long)pos + 1;
    uint32_t wiv = me.niv, k0 = 0, n_out = 0;
    if (cov && n_cigar > 0) { const uint32_t t = src.ld32(cig_o) & 15u; if (t == C_S || t == C_H) k0 = 1; }
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t cg = src.ld32(cig_o + 4ull * k), t = cg & 15u, l = cg >> 4;
        if (cov && k >= k0) {                                                                 // qaCompute.cpp:530-552
            if (t == C_M) {
                if (pp >= L) { if (L >= 1) { A.cov_tid[wiv] = tid; A.cov_beg[wiv] = (int32_t)L; A.cov_end[wiv] = (int32_t)(L - 1); ++wiv; } }
                else if (pp < L - 1 && l > 0u) { A.cov_tid[wiv] = tid; A.cov_beg[wiv] = (int32_t)pp; A.cov_end[wiv] = (int32_t)(pp + l); ++wiv; }      // (the kept ones only: msnv_measure_reads / measure_one counts the same)
            }
            pp += l;
        }
        if (cg_match(t)) {
            if (pile) for (uint32_t off = 0, n = 0; off < l; off += n) {
                const long long gl = rp + off;
                const uint32_t g = (uint32_t)gl;
                const uint32_t to_tile = TILE - (uint32_t)(gl % TILE);
                n = SEG_MAX < l - off ? SEG_MAX : l - off;
                n = n < to_tile ? n : to_tile;
                const uint32_t tl = (uint32_t)(gl / TILE);
                if (!have_ftile) { ftile = tl; have_ftile = true; }
                const uint32_t dst = A.in_order ? w : (tl == ftile ? d_own++ : d_next++);
                ReadHdr h;
                h.gpos = g; h.seqoff = so; h.cig = n; h.meta = META_PILEUP_OK | mapq << 16;
                A.hdr[dst] = h; A.ptid[dst] = tid; A.pend[dst] = (int32_t)(g + n);      // (the piece's depth: msnv_depth2)
                PieceDesc D;
                D.seq_o = (uint32_t)seq_o; D.qual_o = (uint32_t)qual_o; D.q0 = noseq ? 0xffffffffu : q + off; D.so = so;
                unsigned long long ref_nib; uint32_t ref_left;
                const long long left = c.seq_len - gl;
                if (c.seq_len >= 0 && gl >= 0 && left > 0) { ref_nib = c.pref_off + (unsigned long long)gl; ref_left = (uint32_t)(left < 0xffffffffll ? left : 0xffffffffll); }
                else { ref_nib = c.seq_len >= 0 ? ~1ull : ~0ull; ref_left = 0; }              // ~1: a FASTA record exists but holds nothing here (sampled, nothing to compare)
                D.ref_lo = (uint32_t)ref_nib; D.ref_hi = (uint32_t)(ref_nib >> 32); D.ref_left = ref_left;
                const bool sample_this = ref_nib != ~0ull && ((w - (uint32_t)d.pbase0) & 15u) == 0u;   // one piece in 16: how noisy are these reads?
                D.nf = n | (sample_this ? 256u : 0u) | (to_tile - n < 3u ? to_tile - n : 3u) << 9;
                if (n_out == 0) *first_slot = D; else more_slots[n_out - 1u] = D;
                ++n_out; ++w; so += stored_bytes(n);
            }
            rp += l; q += l;
        } else {
            if (cg_ref(t)) rp += l;
            if (cg_query(t)) q += l;
        }
    }
}
__global__ __launch_bounds__(256) void msnv_emit_block(const EmitArgs A) {
    __shared__ uint4 win[EW_BYTES / 16 + 4];                       // (+ 64 bytes: a lane's last loads run past its piece)
    __shared__ uint4 img_seq[EO_BYTES / 16 + 2];                   // (+ 32 bytes: a lane ORs five words from any byte)
    __shared__ uint4 img_flag[EO_BYTES / 64 + 2];
    __shared__ PieceDesc s_desc[PB + EQ_CAP];
    __shared__ unsigned long long s_mm[2];
    __shared__ uint32_t s_misc[2];                                 // [0] further pieces of the block, [1] "not this kernel's"
    const uint32_t b = blockIdx.x, tid = threadIdx.x, i0 = b * PB;
    const uint32_t nrec = A.n_rec - i0 < PB ? A.n_rec - i0 : PB;
    const unsigned long long lo = A.rec_off[i0] & ~15ull, hi = A.rec_off[i0 + nrec];      // (entry n_rec: the end of the round's records)
    const bool direct = hi - lo > EW_BYTES;
    const uint32_t smp_first = A.rec_sample[i0], smp_last = A.rec_sample[i0 + nrec - 1u];
    const RecCnt base = A.r_pre[i0], next = A.r_pre[i0 + nrec];
    // ---- the first wavefront's lanes: what their record needs of the per-record columns (asked for together with the window)
    const uint32_t i = i0 + (tid < nrec ? tid : 0u);
    uint8_t f = 0; uint16_t depth = 0; unsigned long long ro = 0; RecCnt pre{}; uint32_t my_pieces = 0;
    if (tid < PB) { f = A.r_flags[i]; ro = A.rec_off[i]; pre = A.r_pre[i]; if (tid < nrec) my_pieces = A.r_pre[i + 1u].npiece - pre.npiece; }
    // ---- the block's bytes into LDS
    if (!direct) {
        const uint32_t n16 = (uint32_t)((hi - lo + 15) >> 4);
        uint4 v[EW_BYTES / 16 / 256];
#pragma unroll
        for (uint32_t k = 0; k < EW_BYTES / 16 / 256; ++k) { const uint32_t c = tid + 256u * k; v[k] = c < n16 ? *reinterpret_cast<const uint4 *>(A.raw + lo + 16ull * c) : make_uint4(0, 0, 0, 0); }
#pragma unroll
        for (uint32_t k = 0; k < EW_BYTES / 16 / 256; ++k) { const uint32_t c = tid + 256u * k; if (c < n16 + 4u) win[c] = v[k]; }
    }
    // ---- the image of the block's stretch of its sample's columns: one sample, a stretch the image holds
    const unsigned long long sb0 = A.samp_sbase0[smp_first];
    const unsigned long long a0 = base.seqb - sb0, b0 = next.seqb - sb0;             // the block's pieces own bytes [a0, b0) of the sample's seq column
    const uint32_t a16 = (uint32_t)a0 & ~15u;
    const bool image = !direct && smp_first == smp_last && b0 - a16 <= EO_BYTES && b0 > a0;
    if (image) {
        for (uint32_t c = tid; c < EO_BYTES / 16 + 2; c += 256u) img_seq[c] = make_uint4(0, 0, 0, 0);
        if (tid < EO_BYTES / 64 + 2) img_flag[tid] = make_uint4(0, 0, 0, 0);
    }
    if (tid == 0) { s_mm[0] = 0ull; s_mm[1] = 0ull; }
    __syncthreads();
    LdsSrcK lsrc; lsrc.w = reinterpret_cast<const uint32_t *>(win);
    const DpSampleDst d = A.dst[smp_first];
    if (tid < PB) {
        // ---- phase A (one wavefront)
        // (its group's words and its contig are asked for here, not under the window's loads: the window's way into LDS would wait for
        // these chains of dependent loads -- measured: 2.24 -> 2.38 ms)
        uint32_t more = my_pieces ? my_pieces - 1u : 0u, more_pre = more;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(more_pre, o); if ((int)tid >= o) more_pre += y; }
        const uint32_t more_all = __shfl(more_pre, 63);
        more_pre -= more;
        bool odd = !image || more_all > EQ_CAP || A.force_slow;                   // (no pieces at all: nothing for the image form to do either -- the slow kernel writes the intervals)
        if (!odd && tid < nrec) {
            // a CIGAR that may live in the CG field (placeholder `<l_seq>S...`: hostio.cpp rec_parse) is walked by rec_load, from global memory
            const unsigned long long o = ro - lo;
            const uint32_t fn = lsrc.ld32(o + 16), l_name = lsrc.ld32(o + 12) & 0xffu;
            const int32_t l_seq = (int32_t)lsrc.ld32(o + 20);
            if ((fn & 0xffffu) > 0) { const uint32_t c0 = lsrc.ld32(o + 36 + l_name); odd = (c0 & 15u) == C_S && (int32_t)(c0 >> 4) == l_seq; }
        }
        odd = __any(odd);
        if (tid == 0) {
            s_misc[0] = more_all; s_misc[1] = odd ? 1u : 0u;
            if (odd) A.slow[1u + atomicAdd(A.slow, 1u)] = b;
        }
        if (!odd) {
            DpContig ctg_mine{}; uint2 pf = make_uint2(0u, 0u), pe = make_uint2(0u, 0u);
            if (tid < nrec) {
                if ((f & RF_PILE) && !A.in_order) {
                    const uint32_t gi = (uint32_t)A.rg[i] - 1u;
                    pf = A.grp_pre[gi]; pe = A.grp_pre[gi + 1u];
                }
                if (f & (RF_PILE | RF_COV)) ctg_mine = A.ctg[(int32_t)lsrc.ld32(ro - lo + 4)];
            }
            if (tid < nrec) emit_walk(A, lsrc, ro - lo, pre, f, depth, d, sb0, ctg_mine, pf, pe, &s_desc[tid], &s_desc[PB + more_pre]);
            else { PieceDesc none{}; s_desc[tid] = none; }
        }
    }
    __syncthreads();
    if (s_misc[1]) return;
    // ---- phase B: four lanes a piece, 32 bases a lane, into the image
    LdsOut lout; lout.seq_w = reinterpret_cast<uint32_t *>(img_seq); lout.flag_w = reinterpret_cast<uint32_t *>(img_flag); lout.a16 = a16;
    {
        const uint32_t n_desc = PB + s_misc[0], sub = tid & 3u, j0 = 32u * sub;
        for (uint32_t t = tid >> 2; t < n_desc; t += 64u) {
            const PieceDesc D = s_desc[t];
            const uint32_t n = D.nf & 0xffu;
            if (!n) continue;
            const bool sample_this = (D.nf & 256u) != 0u;
            const uint32_t sb = stored_bytes(n);
            const uint32_t st = 2u * sb > j0 ? (2u * sb - j0 < 32u ? 2u * sb - j0 : 32u) : 0u;    // stored nibbles of this lane (a multiple of 4)
            const uint32_t have = n > j0 ? (n - j0 < 32u ? n - j0 : 32u) : 0u;                     // ... of which real bases
            uint64_t o0, o1; uint32_t bits, mm;
            piece_lane(lsrc, D.seq_o, D.qual_o, D.q0, j0, have, (unsigned long long)D.ref_hi << 32 | D.ref_lo, D.ref_left, A.pref4, A.P, d.cut_marks, sample_this && have, (D.nf >> 9) & 3u,
                       o0, o1, bits, mm);
            lout.put(d, D.so, sub, sb, st, o0, o1, bits, 0u);
            if (sample_this) {                                         // mismatch sample: sum over the 4 lanes of a piece, one LDS atomic per sampled piece
                mm += __shfl_down(mm, 2, 4); mm += __shfl_down(mm, 1, 4);
                if (sub == 0) { atomicAdd(&s_mm[0], (unsigned long long)n); if (mm) atomicAdd(&s_mm[1], (unsigned long long)mm); }
            }
        }
    }
    __syncthreads();
    if (tid == 0 && s_mm[0]) {
        DpAcc &a = A.acc[(size_t)smp_first * ACC_COPIES + (blockIdx.x % ACC_COPIES)];
        atomicAdd(&a.mm_bases, s_mm[0]);
        if (s_mm[1]) atomicAdd(&a.mm, s_mm[1]);
    }
    // ---- the image out: whole 16-byte pieces of the columns where the block owns all of them, its own bytes / half bytes at the two ends
    {
        const uint32_t n16 = ((uint32_t)b0 - a16 + 15u) >> 4;
        for (uint32_t c = tid; c < n16; c += 256u) {
            const uint32_t g0 = a16 + 16u * c;                      // byte of the seq column
            const uint4 v = img_seq[c];
            if (g0 >= (uint32_t)a0 && g0 + 16u <= (uint32_t)b0) *reinterpret_cast<uint4 *>(d.seq + g0) = v;
            else {
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (uint32_t k = 0; k < 16u; k += 2u) if (g0 + k >= (uint32_t)a0 && g0 + k < (uint32_t)b0) { const uint16_t h = (uint16_t)(w[k >> 2] >> (8u * (k & 3u))); __builtin_memcpy(d.seq + g0 + k, &h, 2); }      // (pieces start and end on 2 bytes)
            }
        }
        // flags: bits [2 a0, 2 b0) of the flag column = bytes from a16 / 4; a byte at an end may be half a neighbour's
        const uint32_t fa = 2u * (uint32_t)a0, fbe = 2u * (uint32_t)b0, w_n = (fbe - 2u * a16 + 31u) >> 5;
        const uint32_t *fw = reinterpret_cast<const uint32_t *>(img_flag);
        for (uint32_t c = tid; c < w_n; c += 256u) {
            const uint32_t bit0 = 2u * a16 + 32u * c, v = fw[c];
            uint8_t *gp = d.qual + (bit0 >> 3);
            if (bit0 >= fa && bit0 + 32u <= fbe) __builtin_memcpy(gp, &v, 4);
            else for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t lo_b = bit0 + 8u * k, byte = (v >> (8u * k)) & 0xffu;
                if (lo_b >= fa && lo_b + 8u <= fbe) gp[k] = (uint8_t)byte;
                else if (lo_b + 8u > fa && lo_b < fbe && byte) or_byte(gp + k, byte);      // half a byte is this block's (the other half is zero in the image)
            }
        }
    }
}
// The blocks the quick form left (listed in A.slow): four lanes per record from global memory, piece after piece, byte-granular stores with
// the nibbles shared between neighbours OR-ed in atomically -- round 4's route, which takes everything (records longer than the LDS window,
// blocks that hold two samples, CIGARs in the CG field).
__global__ __launch_bounds__(256) void msnv_emit_block_slow(const EmitArgs A) {
    __shared__ RecCnt s_pre[PB];
    const uint32_t n_list = A.slow[0], tid = threadIdx.x;
    GlbSrcK gsrc; gsrc.p = A.raw;
    GlbOut gout;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t b = A.slow[1u + li], i0 = b * PB;
        const uint32_t nrec = A.n_rec - i0 < PB ? A.n_rec - i0 : PB;
        const uint32_t r = tid >> 2, sub = tid & 3u, i = i0 + (r < nrec ? r : 0u);
        const uint8_t f = A.r_flags[i]; const uint32_t smp = A.rec_sample[i]; const uint16_t depth = 0; const unsigned long long ro = A.rec_off[i];
        __syncthreads();                                            // (the list's previous block has read s_pre)
        if (tid < 64) s_pre[tid] = A.r_pre[i0 + (tid < nrec ? tid : 0u)];
        __syncthreads();
        if (r < nrec) emit_record(A, gsrc, gout, ro, s_pre[r], sub, f, smp, depth, i);
    }
}

// behind the last piece of every sample: 32 bytes of N and their flags (pack.cpp: pack_sample's tail padding)
__global__ void msnv_emit_tail(const DpSampleDst *dst, const unsigned long long *seq_bytes, uint32_t n_samples, DpParams P) {
    const uint32_t s = blockIdx.x, t = threadIdx.x;      // 64 threads
    if (s >= n_samples) return;
    const unsigned long long nb = seq_bytes[s];          // without the tail
    if (t < 32 + (uint32_t)((16u - ((nb + 32u) & 15u)) & 15u)) dst[s].seq[nb + t] = 0xff;      // ... and on to the next 16-byte boundary, where the next sample's column starts
    if (P.c_eff > 0 || P.all_low) {                      // 64 flags from bit 2 * nb (a multiple of 4)
        const unsigned long long b0 = 2ull * nb;
        if (t < 16) or_byte(dst[s].qual + ((b0 + 4ull * t) >> 3), ((b0 + 4ull * t) & 4ull) ? 0xf0u : 0x0fu);
    }
}

// ------------------------------------------------------------------------------------------ tile order of the headers
__device__ __forceinline__ uint32_t piece_sample(const DpSampleDst *dst, uint32_t n_samples, uint32_t pc) {      // last sample whose first piece is at or before pc
    uint32_t a = 0, b = n_samples;
    while (b - a > 1) { const uint32_t m = (a + b) / 2; if ((uint32_t)dst[m].pbase0 <= pc) a = m; else b = m; }
    return a;
}
__global__ void msnv_tile_keys(const ReadHdr *hdr, const int32_t *ptid, const DpSampleDst *dst, uint32_t n_samples, uint32_t n, uint32_t tid_bits,
                               unsigned long long *keys, uint32_t *idx, uint32_t *unsorted) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = ((unsigned long long)piece_sample(dst, n_samples, i) << tid_bits | (uint32_t)ptid[i]) << 21 | (hdr[i].gpos / TILE);
    keys[i] = k; idx[i] = i;
    if (i > 0) {
        const unsigned long long kp = ((unsigned long long)piece_sample(dst, n_samples, i - 1) << tid_bits | (uint32_t)ptid[i - 1]) << 21 | (hdr[i - 1].gpos / TILE);
        if (kp > k) *unsorted = 1u;
    }
}
__global__ void msnv_gather_pieces(const uint32_t *idx, uint32_t n, const ReadHdr *hdr, const int32_t *ptid, const int32_t *pend, const uint16_t *pdepth,
                                   ReadHdr *hdr2, int32_t *ptid2, int32_t *pend2, uint16_t *pdepth2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = idx[i];
    hdr2[i] = hdr[j]; ptid2[i] = ptid[j]; pend2[i] = pend[j]; pdepth2[i] = pdepth[j];
}

// ------------------------------------------------------------------------------------------ (sample, contig, tile) runs of the sorted pieces
struct DevPairRec { uint32_t sample; int32_t tid; uint32_t tile, start, maxd; };     // start: piece index in the round
__global__ void msnv_pair_flags(const unsigned long long *keys, uint32_t n, uint32_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
__global__ void msnv_pair_starts(const unsigned long long *keys, const uint32_t *flag, const uint32_t *pid_incl, uint32_t n, uint32_t tid_bits, DevPairRec *recs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const unsigned long long k = keys[i];
    DevPairRec r;
    r.tile = (uint32_t)(k & 0x1fffffu); r.tid = (int32_t)((k >> 21) & ((1ull << tid_bits) - 1ull)); r.sample = (uint32_t)(k >> (21u + tid_bits)); r.start = i; r.maxd = 0;
    recs[pid_incl[i] - 1u] = r;
}
__global__ void msnv_pair_maxd(DevPairRec *recs, uint32_t n_pairs, uint32_t n_pieces, const uint16_t *depth) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t lo = recs[p].start, hi = p + 1 < n_pairs ? recs[p + 1].start : n_pieces;
    uint32_t m = 0;
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t d = depth[i]; m = d > m ? d : m; }
    recs[p].maxd = m;
}

// ------------------------------------------------------------------------------------------ host side
// contig table (small: goes up at once, the record scan's walk reads it) ...
int build_contigs(msnv_dataset &ds) {
    DevPackTables &t = ds.dp;
    if (t.contigs) return MSNV_OK;
    const size_t NC = ds.names.size();
    std::vector<DpContig> ct(NC);
    uint64_t nib = 0;
    for (size_t c = 0; c < NC; ++c) {
        DpContig &d = ct[c];
        d.len = ds.lengths[c]; d.seq_len = ds.has_seq[c] ? (long long)ds.seqs[c].size() : -1;
        d.bed_beg = ds.bed_beg[c]; d.bed_end = ds.bed_end[c]; d.sel = ds.sel[c]; d.pad = 0; d.pref_off = nib;
        if (ds.sel[c] && ds.has_seq[c]) nib += (ds.seqs[c].size() + 7) & ~(size_t)7;
    }
    t.pref_words = nib / 8 + 8;                                  // (msnv_emit_block reads five words from a lane's first position)
    if (int rc = dev_alloc(&t.contigs, std::max<size_t>(1, NC) * sizeof(DpContig), nullptr)) return rc;
    if (int rc = dev_alloc((void **)&t.overhang, (std::max<size_t>(1, NC) + 1) * sizeof(int32_t), nullptr)) return rc;
    // (plain blocking copies on the null stream: fresh buffers, nothing of the context's stream to order against)
    if (NC) HIP_TRY(hipMemcpy(t.contigs, ct.data(), NC * sizeof(DpContig), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(t.overhang, 0, (std::max<size_t>(1, NC) + 1) * sizeof(int32_t)));
    HIP_TRY(hipStreamSynchronize(nullptr));
    t.any_overhang = reinterpret_cast<uint32_t *>(t.overhang + std::max<size_t>(1, NC));
    return MSNV_OK;
}
// ... and the packed FASTA of the selected contigs (the emit kernels read it: built on a thread of its own beside the round's first kernels)
int build_tables(msnv_dataset &ds) {
    DevPackTables &t = ds.dp;
    if (t.ready) return MSNV_OK;
    const size_t NC = ds.names.size();
    std::vector<uint64_t> pref_off(NC, 0);
    {
        uint64_t nib = 0;
        for (size_t c = 0; c < NC; ++c) { pref_off[c] = nib; if (ds.sel[c] && ds.has_seq[c]) nib += (ds.seqs[c].size() + 7) & ~(size_t)7; }
    }
    if (int rc = dev_alloc((void **)&t.pref4, t.pref_words * sizeof(uint32_t), nullptr)) return rc;
    // the FASTA characters of the selected contigs -> nt16 codes, 8 per word, and lower-case bits, 32 per word: once per dataset, kept on the
    // host too (finalize lays them out by tile without going back to the characters); big references are cut into pieces for the host threads
    static const struct Tab { uint8_t code[256], lc[256]; Tab() { for (int c = 0; c < 256; ++c) { code[c] = nt16_of_char((unsigned char)c); lc[c] = (c == 'a' || c == 'c' || c == 'g' || c == 't') ? 1 : 0; } } } tab;
    t.h_codes.assign(t.pref_words, 0xffffffffu);
    t.h_code_off.assign(NC, ~0ull); t.h_lc_off.assign(NC, ~0ull);
    uint64_t lc_words = 0;
    struct Job { size_t c; uint64_t w0, w1; };                   // words [w0, w1) of contig c
    std::vector<Job> jobs;
    for (size_t c = 0; c < NC; ++c) {
        if (!ds.sel[c] || !ds.has_seq[c]) continue;
        t.h_code_off[c] = pref_off[c] / 8; t.h_lc_off[c] = lc_words;
        const uint64_t nw = (ds.seqs[c].size() + 7) / 8;
        lc_words += (ds.seqs[c].size() + 31) / 32;
        for (uint64_t w = 0; w < nw; w += 1u << 14) jobs.push_back(Job{c, w, std::min<uint64_t>(nw, w + (1u << 14))});
    }
    t.h_lc.assign(lc_words + 1, 0u);
    auto run_job = [&](const Job &j) {
        const std::string &sq = ds.seqs[j.c];
        uint32_t *cw = t.h_codes.data() + t.h_code_off[j.c];
        uint32_t *lw = t.h_lc.data() + t.h_lc_off[j.c];
        for (uint64_t w = j.w0; w < j.w1; ++w) {
            const size_t i0 = 8 * w, lim = std::min<size_t>(8, sq.size() - i0);
            uint32_t v = 0xffffffffu, l = 0;
            for (size_t k = 0; k < lim; ++k) { const unsigned char ch = (unsigned char)sq[i0 + k]; v = (v & ~(0xfu << (4 * k))) | (uint32_t)tab.code[ch] << (4 * k); l |= (uint32_t)tab.lc[ch] << k; }
            cw[w] = v;
            if (l) reinterpret_cast<uint8_t *>(lw)[w] = (uint8_t)l;          // (8 bases = one byte of the bit column: no two jobs share a byte)
        }
    };
    if (jobs.size() <= 2) for (const Job &j : jobs) run_job(j);
    else {
        std::atomic<size_t> next{0};
        std::vector<std::thread> th;
        const size_t nt = std::min<size_t>(std::min<size_t>(jobs.size() / 2, msnv_default_threads()), jobs.size() < 64 ? 4 : 32);
        for (size_t k = 0; k < nt; ++k) th.emplace_back([&]() { for (;;) { const size_t i = next.fetch_add(1); if (i >= jobs.size()) break; run_job(jobs[i]); } });
        for (auto &x : th) x.join();
    }
    HIP_TRY(hipMemcpy(t.pref4, t.h_codes.data(), t.pref_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    t.ready = true;
    return MSNV_OK;
}

const char *err_text(uint32_t kind) {
    switch (kind) {
        case ERR_MALFORMED: return "malformed BAM record";
        case ERR_TID: return "record refers to a contig the header does not have";
        case ERR_UNSORTED: return "BAM is not coordinate sorted";
        case ERR_QLEN: return "CIGAR and read length disagree";
        default: return "bad record";
    }
}

}  // namespace

// The dataset's pinned block: at least `half` bytes in each of its two halves.  Taken from the context's pool (a fresh dataset of a context
// that has built one before pins nothing); grown only while nothing is in flight into it.  The first half is a round's (DpAcc per sample);
// the second is finalize's result words, sized ONCE per finalize by whichever stage uses them first (devfin.h: FinWords).
int pin_ensure(msnv_dataset &ds, uint64_t half) {
    DevPackTables &T = ds.dp;
    if (T.pin && T.pin_cap / 2 >= half) return MSNV_OK;
    if (int rc = devpack_sync_pending(ds)) return rc;
    msnv_ctx *ctx = ds.ctx;
    if (T.pin) { ctx->pin_pool.emplace_back(T.pin, T.pin_cap); T.pin = nullptr; T.pin_cap = 0; }
    const uint64_t want = std::max<uint64_t>(2 * half, 1ull << 20);
    size_t best = SIZE_MAX;
    for (size_t i = 0; i < ctx->pin_pool.size(); ++i) if (ctx->pin_pool[i].second >= want && (best == SIZE_MAX || ctx->pin_pool[i].second < ctx->pin_pool[best].second)) best = i;
    if (best != SIZE_MAX) { T.pin = ctx->pin_pool[best].first; T.pin_cap = ctx->pin_pool[best].second; ctx->pin_pool.erase(ctx->pin_pool.begin() + (ptrdiff_t)best); return MSNV_OK; }
    HIP_TRY(hipHostMalloc(&T.pin, want, hipHostMallocDefault));
    T.pin_cap = want;
    return MSNV_OK;
}

int devpack_sync_pending(msnv_dataset &ds) {
    DevPackTables &T = ds.dp;
    if (!T.pending.active) return MSNV_OK;
    T.pending.active = false;
    HIP_TRY(hipEventSynchronize((hipEvent_t)T.pending.ev1));
    float ms = 0;
    if (hipEventElapsedTime(&ms, (hipEvent_t)T.pending.ev0, (hipEvent_t)T.pending.ev1) == hipSuccess) T.ms_emit += ms;
    if (T.pending.has_evd) { T.pending.has_evd = false; if (hipEventElapsedTime(&ms, (hipEvent_t)T.pending.evd, (hipEvent_t)T.pending.evd2) == hipSuccess) T.ms_depth += ms; }      // (the quick route's depth stage, on the second stream beside the emit kernels)
    const DpAcc *a = static_cast<const DpAcc *>(T.pin);
    for (size_t s = 0; s < T.pending.n && T.pending.first + s < ds.samples.size(); ++s) {
        SampleCols &sc = ds.samples[T.pending.first + s];
        sc.mm_sampled_bases = a[s].mm_bases; sc.mm_sampled = a[s].mm;
    }
    uint32_t n_slow = 0;
    memcpy(&n_slow, a + T.pending.n, 4);                           // (behind the round's accumulators: launch_emit)
    T.n_emit_slow_blocks += n_slow;
    return MSNV_OK;
}
void devpack_ctx_release(msnv_ctx *ctx) {
    if (!ctx) return;
    for (auto &b : ctx->pin_pool) if (b.first) (void)hipHostFree(b.first);
    ctx->pin_pool.clear();
}

void devpack_release(msnv_dataset &ds) {
    DevPackTables &t = ds.dp;
    if (t.pending.active) { (void)hipDeviceSynchronize(); t.pending.active = false; }
    if (t.pending.ev0) {
        (void)hipEventDestroy((hipEvent_t)t.pending.ev0); (void)hipEventDestroy((hipEvent_t)t.pending.ev1); (void)hipEventDestroy((hipEvent_t)t.pending.evh); (void)hipEventDestroy((hipEvent_t)t.pending.evd);
        (void)hipEventDestroy((hipEvent_t)t.pending.evd2); (void)hipEventDestroy((hipEvent_t)t.pending.evw);
        t.pending.ev0 = t.pending.ev1 = t.pending.evh = t.pending.evd = t.pending.evd2 = t.pending.evw = nullptr;
    }
    // everything of the pack goes back in ONE batch (one wait for the device instead of one per buffer: dev_free_batch)
    std::vector<void *> out;
    auto give = [&](void *p) { if (p) out.push_back(p); };
    devfin_release(t.fin, out);                                     // (finalize's events, the wait for what it left queued, its buffers: devfin.hip)
    give(t.contigs); give(t.pref4); give(t.overhang);
    t.overhang = nullptr; t.any_overhang = nullptr;
    for (DevRound &r : t.rounds) give(r.buf);
    t.rounds.clear();
    for (void *p : t.round_bufs) give(p);
    t.round_bufs.clear();
    for (auto &b : t.scratch) give(b.first);
    t.scratch.clear();
    t.contigs = nullptr; t.pref4 = nullptr; t.ready = false;
    std::vector<uint32_t>().swap(t.h_codes); std::vector<uint32_t>().swap(t.h_lc);
    dev_free_batch(out);
    if (t.pin) {
        if (ds.ctx) ds.ctx->pin_pool.emplace_back(t.pin, t.pin_cap); else (void)hipHostFree(t.pin);
        t.pin = nullptr; t.pin_cap = 0;
    }
}

int Prim::scan32(const uint32_t *in, uint32_t *out, size_t n, bool inclusive_) {
    return inclusive_ ? inclusive(in, out, n, rocprim::plus<uint32_t>()) : exclusive(in, out, 0u, n, rocprim::plus<uint32_t>());
}
int Prim::sort64(unsigned long long *kin, unsigned long long *kout, uint32_t *vin, uint32_t *vout, size_t n, unsigned end_bit) { return sort_pairs(kin, kout, vin, vout, n, end_bit); }

// ------------------------------------------------------------------------------------------ one round of samples through the per-read stage
namespace {
constexpr int TO_CAREFUL = -1;      // a stage's verdict beside MSNV_OK and the error codes: the careful route has to take this round

// Everything one call of devpack_add_round works on.  The stages are member functions; each says what it takes and what it leaves.  Host
// words that an asynchronous copy reads or writes are members here (or lie in the dataset's pinned block) unless the function that queues
// the copy also waits for it: no stage leaves a copy in flight into its own frame.
struct Round {
    // ---- the inputs, and what every stage reads
    msnv_dataset &ds; DevPackTables &T; const msnv_params &MP;
    const size_t first; const uint8_t *const *const streams; const uint64_t *const n_bytes; const size_t S, NC; const bool on_device; const uint8_t *const in_place_base;
    const hipStream_t st; DpParams P{}; const DpContig *ctg = nullptr;
    // the packed FASTA of the selected contigs is built by the first round, on a thread of its own BESIDE the round's first kernels, which
    // do not read it (round 5: 0.4 ms in front of them); the emit kernels do
    Timer tm; ThreadJob tables;
    // work buffers of the round: taken from the dataset's pool in call order (BufPool: grow-only, so a dataset's second round allocates nothing;
    // with guarded allocations -- MSNV_GUARD_ALLOC=1 -- every buffer is exact and fresh); rocPRIM's storage is one slot of it
    BufPool pool; Prim prim; size_t pool_staged = 0;
    // ---- stage(): the streams in place, the quick walk's sub-segments
    ScanResult SR; uint8_t *raw = nullptr; unsigned long long end_all = 0;
    std::vector<SubStream> ss; uint64_t n_sub64 = 0; uint32_t sub_bytes = 0, cap2 = 0; bool quick_possible = false;
    // ---- a front: the records' tables, the round's totals and lasting buffers, the depth stage launched
    bool quick = false;                                          // the route that runs
    uint32_t NR = 0, NPC = 0, NIV = 0, n_runs = 0, n_groups = 0, span_out = SPAN_OUT; uint64_t seqb_total = 0, seq_bound = 0, qual_bound = 0; bool in_order = false;
    DpAcc *d_acc = nullptr; uint32_t *d_misc = nullptr, *d_outl = nullptr; uint8_t *d_cut = nullptr;
    RdTables TB{}; uint32_t *d_recbase = nullptr; unsigned long long *d_send = nullptr;
    uint32_t *d_runfirst = nullptr, *d_runf1 = nullptr, *d_grpfirst = nullptr, *d_grpmd = nullptr; DpRun *d_runs = nullptr; uint2 *d_grppre = nullptr; DevGroupRec *d_groups = nullptr;
    uint32_t fl_h = 0; SubCnt tot_q{}; RecCnt tot_c{}, totals_h{}; uint32_t misc_h[MISC_WORDS] = {0, 0, 0, 0};      // (words of asynchronous copies)
    struct Held {                                                // the round's lasting buffers, the round's until it is known to stand
        void *round_buf = nullptr, *keep_buf = nullptr;
        void drop() { if (round_buf) dev_free(round_buf); if (keep_buf) dev_free(keep_buf); round_buf = keep_buf = nullptr; }
        ~Held() { drop(); }
    } held;
    DevRound keep; uint8_t *r_seq = nullptr, *r_qual = nullptr;
    ReadHdr *w_hdr = nullptr; int32_t *w_tid = nullptr, *w_end = nullptr; uint16_t *w_depth = nullptr;      // where the emit kernels write the headers (keep's, or work buffers first)
    DpSampleSum2 *d_sum = nullptr; unsigned long long *d_ss0 = nullptr, *d_pb = nullptr; uint32_t *d_slow = nullptr; DpSampleDst *d_dst = nullptr;
    // ---- the careful front's work columns and what its sequential edits need
    uint8_t *c_flags0 = nullptr; unsigned long long *c_key = nullptr, *c_sf = nullptr; uint32_t *c_end = nullptr, *c_maxc = nullptr; RecCnt *c_cnt = nullptr, *c_blkcnt = nullptr, *c_blkpre = nullptr;
    uint32_t *d_ovr = nullptr; bool have_ovr = false;
    uint32_t *d_depth0 = nullptr, *d_hot = nullptr, *d_hotn = nullptr, *d_capfail = nullptr;      // (msnv_cap_reads / msnv_token_cut)
    std::vector<uint32_t> dev_cap, dev_tok;                      // samples whose depth cap / token limit the kernels take
    DevBuf o_flag, o_rank, o_skip, o_keys, o_skeys, o_vals, o_svals, o_starts;      // overlapping mates (paired reads only: not from the pool)
    uint32_t n_ovl_reads = 0, n_ovl_groups = 0;
    // ---- the host's side of the round
    std::vector<DpAcc> acc; std::vector<uint8_t> cut_marks, host_sample; std::vector<DpRun> runs; std::vector<DevGroupRec> groups;
    std::vector<DpSampleSum2> sum; std::vector<unsigned long long> piece_bytes; std::vector<uint32_t> rec_base_h;
    uint8_t *pinb = nullptr; uint64_t o_acc = 0, o_sum = 0, o_pb = 0, o_rb = 0, o_misc = 0, o_runs = 0, o_grp = 0;      // the pinned words launch_emit() fills and collect() reads
    std::vector<DevPairRec> prec; uint32_t uns_h = 0, n_pairs_h = 0;

    Round(msnv_dataset &ds_, size_t first_, const uint8_t *const *streams_, const uint64_t *n_bytes_, int n, bool on_device_, const uint8_t *in_place_base_)
        : ds(ds_), T(ds_.dp), MP(ds_.params), first(first_), streams(streams_), n_bytes(n_bytes_), S((size_t)n), NC(ds_.names.size()), on_device(on_device_), in_place_base(in_place_base_),
          st((hipStream_t)ds_.ctx->stream), tm(st), pool{T.scratch}, prim(st), ss(S), acc(S), cut_marks(S, 0), host_sample(S, 0), sum(S + 1), piece_bytes(S) {
        if (!T.ready) {
            const int device = ds.ctx->device;
            msnv_dataset *d = &ds; ThreadJob *job = &tables;
            tables.th = std::thread([d, job, device]() {
                (void)hipSetDevice(device);
                try { job->rc = build_tables(*d); } catch (const std::exception &e) { job->rc = fail_quiet(MSNV_ENOMEM, "device pack tables: %s", e.what()); }
                if (job->rc) job->msg = msnv_last_error();
            });
        }
        P.flag_filter = MP.flag_filter; P.min_mapq = MP.min_mapq; P.count_orphans = MP.count_orphans; P.cov_min_mapq = MP.cov_min_mapq;
        P.max_depth = MP.max_depth; P.token_limit = MP.token_limit; P.ignore_overlaps = MP.ignore_overlaps;
        P.c_eff = std::min(std::max(MP.min_baseq, -127), 127); P.all_low = MP.min_baseq > 127;
        P.n_contigs = (int)NC; P.has_bed = ds.has_bed ? 1 : 0;
    }

    // Takes: the caller's streams.  Leaves: them side by side in one buffer (or where they lie, in HBM), the quick walk's sub-segments, whether
    // the quick route may try, the round's events.  The pool stands at `pool_staged`: everything behind it is a route's.
    int stage() {
        if (int rc = stage_streams(st, ds.ctx->device, pool, streams, n_bytes, S, on_device, SR, in_place_base)) return rc;
        T.wall_upload_s += SR.wall_upload_s; T.raw_bytes += SR.raw_bytes;
        SR.wall_upload_s = 0;
        raw = SR.raw;
        fin_trace("  pack: staged");
        pool_staged = pool.mark();
        ctg = static_cast<const DpContig *>(T.contigs);
        end_all = S ? SR.s_end[S - 1] : 0ull;
        // Two routes to the records' tables.  QUICK (round 6): record boundaries and everything a record decides by itself in ONE walk
        // (msnv_scan_sub2), one wait for the round's totals, then every kernel up to msnv_emit_block launched back to back; what the host
        // learns late -- an error, a sample that needs the host pre-pass, more far-reaching reads than the list holds -- sends the round through
        // the CAREFUL route: round 5's stage-by-stage form (msnv_scan_sub / msnv_scan_segments, msnv_measure_reads, waits between the stages),
        // which also words malformed input and takes the host pre-pass's verdicts.  MSNV_SCAN=segments and MSNV_FRONT=careful force it (tests).
        sub_bytes = knob::scan_sub_bytes(knob::SCAN_SUB_ROUND);   // (per call: tests shrink it; 6 KB: 2.36 -> 2.04 ms of scan + measure on the benchmark shape against 4 KB -- fewer entry guesses --, 8 KB the same)
        const bool quick_wanted = !knob::scan_segments() && !knob::front_careful();
        for (size_t s = 0; s < S; ++s) { ss[s] = SubStream{SR.s_beg[s], SR.s_end[s], (uint32_t)n_sub64, 0u}; n_sub64 += std::max<uint64_t>(1, (n_bytes[s] + sub_bytes - 1) / sub_bytes); }
        cap2 = sub_bytes / 48u + 2u;                              // slots per sub-segment (a sub-segment of more, shorter records takes the careful route)
        quick_possible = quick_wanted && S > 0 && sub_bytes <= 8192 && n_sub64 < 0x7ffffff0ull && n_sub64 * cap2 < 0xfffffff0ull;
        if (!T.pending.ev0) {
            hipEvent_t a = nullptr, b = nullptr, c = nullptr, d = nullptr, e = nullptr, f = nullptr;
            HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b)); HIP_TRY(hipEventCreate(&c)); HIP_TRY(hipEventCreate(&d)); HIP_TRY(hipEventCreate(&e)); HIP_TRY(hipEventCreate(&f));
            T.pending.ev0 = a; T.pending.ev1 = b; T.pending.evh = c; T.pending.evd = d; T.pending.evd2 = e; T.pending.evw = f;
        }
        return MSNV_OK;
    }

    // A route begins: whatever a route before it held goes back (its kernels have been waited for: collect()), the pool stands at
    // `pool_staged` again, the accumulators are cleared.
    int begin_route(bool quick_route) {
        quick = quick_route;
        held.drop();
        pool.rewind(pool_staged);
        T.pending.has_evd = false;
        d_acc = pool.take<DpAcc>(S * ACC_COPIES);
        d_misc = pool.take<uint32_t>(MISC_WORDS);
        d_outl = pool.take<uint32_t>(CAP_OUT);
        d_cut = pool.take<uint8_t>(S);
        if (pool.rc) return pool.rc;
        if (int rc = prim.bind(pool, 1u << 20)) return rc;        // rocPRIM's temporary storage (grown when a call asks for more)
        hipLaunchKernelGGL(msnv_acc_init, grid_for(S * ACC_COPIES, 256), dim3(256), 0, st, d_acc, (uint32_t)(S * ACC_COPIES));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(d_misc, 0, MISC_WORDS * 4, st));
        span_out = SPAN_OUT; n_runs = n_groups = 0; seqb_total = 0; TB = RdTables{};
        d_ovr = d_depth0 = d_hot = d_hotn = d_capfail = nullptr; have_ovr = false;
        std::fill(misc_h, misc_h + MISC_WORDS, 0u);
        std::fill(host_sample.begin(), host_sample.end(), 0); std::fill(cut_marks.begin(), cut_marks.end(), 0);
        return MSNV_OK;
    }

    // The round's lasting buffers and the layout's small tables, once the round's totals are known (NPC, NIV, seqb_total, in_order).  The
    // round's columns: per sample its pieces + 32 tail bytes, starting on 16 bytes, and one flag bit per nibble of them; the samples' shares
    // are laid out on the device (msnv_sample_layout), the buffer is sized by the round's seq bytes + the most the tails and the rounding add.
    int alloc_round_buffers() {
        held.drop();
        seq_bound = (seqb_total + (uint64_t)S * 48ull + 15ull) & ~15ull; qual_bound = seq_bound / 4;
        const uint64_t NPCa = (uint64_t)NPC + 1, NB_ = ((uint64_t)NR + PB - 1) / PB;
        if (int rc = dev_alloc(&held.round_buf, seq_bound + COL_PAD + qual_bound + 64, nullptr)) return rc;
        r_seq = static_cast<uint8_t *>(held.round_buf); r_qual = r_seq + seq_bound + COL_PAD;
        {
            const uint64_t lo = seqb_total & ~15ull;              // (from the lowest place the columns can end to the flags: N -- the exact end is the device's)
            HIP_TRY(hipMemsetAsync(r_seq + lo, 0xff, seq_bound + COL_PAD - lo, st));
            HIP_TRY(hipMemsetAsync(r_qual, 0, qual_bound + 64, st));
        }
        keep = DevRound{};
        {   // what stays in HBM of the round besides the columns: headers (tile order) and intervals, for finalize -- written where they stay
            const uint64_t b_hdr = (uint64_t)NPC * sizeof(ReadHdr), b_4 = (((uint64_t)NPC * 4) + 15) & ~15ull, b_2 = (((uint64_t)NPC * 2) + 15) & ~15ull, b_iv = (((uint64_t)NIV * 4) + 15) & ~15ull;
            if (int rc = dev_alloc(&held.keep_buf, b_hdr + 2 * b_4 + b_2 + 3 * b_iv + 64, nullptr)) return rc;
            uint8_t *q = static_cast<uint8_t *>(held.keep_buf);
            keep.buf = held.keep_buf;
            keep.hdr = reinterpret_cast<ReadHdr *>(q); q += b_hdr;
            keep.tid = reinterpret_cast<int32_t *>(q); q += b_4;
            keep.end = reinterpret_cast<int32_t *>(q); q += b_4;
            keep.depth = reinterpret_cast<uint16_t *>(q); q += b_2;
            keep.cov_tid = reinterpret_cast<int32_t *>(q); q += b_iv;
            keep.cov_beg = reinterpret_cast<int32_t *>(q); q += b_iv;
            keep.cov_end = reinterpret_cast<int32_t *>(q);
            keep.n_pieces = NPC; keep.n_iv = NIV; keep.first_sample = first;
            keep.col_buf = held.round_buf; keep.col_seq = r_seq; keep.col_qual = r_qual; keep.seq_total = 0; keep.n_samples = S;
        }
        d_sum = pool.take<DpSampleSum2>(S + 1);
        d_ss0 = pool.take<unsigned long long>(S + 1);
        d_dst = pool.take<DpSampleDst>(S);
        d_pb = pool.take<unsigned long long>(S);
        d_slow = pool.take<uint32_t>(NB_ + 2);
        // (the general route keeps the headers in file order first: work buffers, sorted into `keep` by tile_pairs())
        w_hdr = keep.hdr; w_tid = keep.tid; w_end = keep.end; w_depth = keep.depth;
        if (in_order) {
            w_hdr = pool.take<ReadHdr>(NPCa);
            w_tid = pool.take<int32_t>(NPCa);
            w_end = pool.take<int32_t>(NPCa);
            w_depth = pool.take<uint16_t>(NPCa);
        }
        return pool.rc;
    }
    // the run and group tables' buffers, once their counts are known
    int take_run_group_tables() {
        d_runfirst = pool.take<uint32_t>((uint64_t)n_runs + 1);
        d_runf1 = pool.take<uint32_t>((uint64_t)n_runs + 1);
        d_runs = pool.take<DpRun>((uint64_t)n_runs + 1);
        d_grpfirst = pool.take<uint32_t>((uint64_t)n_groups + 2);
        d_grpmd = pool.take<uint32_t>(2 * ((uint64_t)n_groups + 1));
        d_grppre = pool.take<uint2>((uint64_t)n_groups + 2);
        d_groups = pool.take<DevGroupRec>((uint64_t)n_groups + 1);
        return pool.rc;
    }
    // depth at every read start (written to the pieces' header slots), the run and group tables: launched on `sx`, not waited for.  Needs
    // the groups' places (msnv_group_pre2) and the round's buffers.
    int launch_depth_stage(hipStream_t sx) {
        HIP_TRY(hipMemsetAsync(d_runf1, 0xff, ((uint64_t)n_runs + 1) * 4, sx));
        HIP_TRY(hipMemsetAsync(d_grpmd, 0, 2 * ((uint64_t)n_groups + 1) * 4, sx));
        if (d_hotn) HIP_TRY(hipMemsetAsync(d_hotn, 0, 4, sx));
        if (NR) hipLaunchKernelGGL(msnv_depth2, grid_for(NR, 256), dim3(256), 0, sx, NR, TB.rd, TB.r_flags, TB.r_rg, TB.r_pre, TB.r_ftile, have_ovr ? d_ovr : nullptr, P, d_misc + MISC_SPAN, d_outl,
                                   d_misc + MISC_NOUT, w_depth, d_grppre, in_order ? 1u : 0u, d_runfirst, d_runf1, d_grpfirst, d_grpmd, d_acc, d_depth0, d_hot, d_hotn);
        if (n_runs) hipLaunchKernelGGL(msnv_run_table2, grid_for(n_runs, 256), dim3(256), 0, sx, n_runs, d_runfirst, d_runf1, TB.rd, d_runs);
        hipLaunchKernelGGL(msnv_group_table2, grid_for((uint64_t)n_groups + 1, 256), dim3(256), 0, sx, n_groups, NR, d_grpfirst, TB.r_pre, TB.rd, TB.r_ftile, d_grpmd, (uint2 *)nullptr, d_groups);
        HIP_TRY(hipGetLastError());
        return MSNV_OK;
    }
    // errors, in record order (what the host stage's sequential walk would have met first)
    int check_errors() const {
        for (size_t s = 0; s < S; ++s) {
            const unsigned long long e = acc[s].err;
            if (e != ~0ull) {
                const uint32_t kind = (uint32_t)(e & 7u); const unsigned long long idx = (e >> 3) - rec_base_h[s];
                return fail(MSNV_EFORMAT, "%s (sample %zu of the batch, record %llu)", err_text(kind), s, idx);
            }
            if (!SR.bad_off.empty() && SR.bad_off[s] != ~0ull) return fail(MSNV_EFORMAT, "malformed BAM record at byte %llu", SR.bad_off[s]);
        }
        return MSNV_OK;
    }

    // ================================================================ QUICK: one walk, one wait
    // Takes: the staged streams.  Leaves: the records' tables (TB), the round's totals and buffers, msnv_scan_write2 .. msnv_acc_fold queued on
    // the stream and the depth stage on the second -- or TO_CAREFUL, with nothing of the round allocated yet.
    int front_quick() {
        if (int rc = begin_route(true)) return rc;
        SubWalk W(S, (uint32_t)n_sub64, sub_bytes, cap2);
        const uint32_t n_sub = W.n_sub;
        W.take(pool);
        auto *d_slots = pool.take<Slot>((uint64_t)n_sub * cap2 + 1);
        auto *d_info = pool.take<SubInfo>((uint64_t)n_sub + 1);
        auto *d_subcnt = pool.take<SubCnt>((uint64_t)n_sub + 1);
        auto *d_subbase = pool.take<SubCnt>((uint64_t)n_sub + 1);
        auto *d_bflag = pool.take<uint8_t>((uint64_t)n_sub + 1);
        d_recbase = pool.take<uint32_t>(S + 1);
        d_send = pool.take<unsigned long long>(S);
        if (pool.rc) return pool.rc;
        fin_trace("  pack: quick buffers");
        tm.start();
        if (int rc = W.upload(st, ss, SR.s_end, d_send)) return rc;
        hipLaunchKernelGGL(msnv_scan_sub2, grid_for(n_sub, 256), dim3(256), 0, st, raw, W.d_ss, (uint32_t)S, n_sub, sub_bytes, cap2, (int)NC, ctg, P, W.d_first, W.d_stop, W.d_cnt, W.d_delta, d_slots, d_info, W.d_fl);
        HIP_TRY(hipGetLastError());
        size_t need = 0;                                          // both scans' storage before either is queued
        if (int rc = W.scan_stops(prim, &need)) return rc;
        if (int rc = prim.exclusive(d_subcnt, d_subbase, SubCnt{}, (size_t)n_sub + 1, SubCntSum(), &need)) return rc;
        if (int rc = prim.room(need)) return rc;
        auto fix = [&]() {
            hipLaunchKernelGGL(msnv_scan_fix2, grid_for(S, 64), dim3(64), 0, st, raw, W.d_ss, (uint32_t)S, sub_bytes, cap2, ctg, P, W.d_first, W.d_stop, W.d_stopmax, W.d_cnt, W.d_delta, d_slots, d_info, W.d_firstbad, W.d_fl);
        };
        // behind the repair: the boundaries, and the scan whose last entry holds the round's totals -- all of it queued before the pass's ONE wait
        auto after = [&]() -> int {
            hipLaunchKernelGGL(msnv_sub_bounds, grid_for((uint64_t)n_sub + 1, 256), dim3(256), 0, st, W.d_ss, (uint32_t)S, n_sub, W.d_cnt, d_info, d_subcnt, d_bflag);
            HIP_TRY(hipGetLastError());
            if (int rc = prim.exclusive(d_subcnt, d_subbase, SubCnt{}, (size_t)n_sub + 1, SubCntSum())) return rc;
            HIP_TRY(hipMemcpyAsync(&tot_q, d_subbase + n_sub, sizeof(SubCnt), hipMemcpyDeviceToHost, st));
            return MSNV_OK;
        };
        if (int rc = W.settle(st, prim, fix, after, fl_h, T.n_scan_redone)) return rc;
        T.ms_scan += tm.stop();
        fin_trace("  pack: scan + measure, totals (wait)");
        const SubCnt &tot = tot_q;
        if (fl_h) { T.n_scan_redone += 1; return TO_CAREFUL; }       // a chain that breaks, a sub-segment with more records than slots: the careful route takes (and words) it
        if (tot.odd) { T.n_quick_redone += 1; return TO_CAREFUL; }   // the walk stands, but a place does not fit its slot field or two contigs overhang in one sub-segment: a round the quick route hands back
        if (SR.raw_bytes / 36 > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 records in one round of the device pack");
        // paired reads: the candidates of the overlapping-mate tweak are grouped, and the samples that need the host pre-pass known, before
        // anything is emitted -- the careful route does all of that; the quick route takes the rounds without candidates
        if (!MP.ignore_overlaps && tot.ovl >= 2) return TO_CAREFUL;
        NR = tot.rec; NPC = tot.npiece; NIV = tot.niv; n_runs = tot.runs; n_groups = tot.grps; seqb_total = tot.seqb;
        in_order = tot.sort != 0 || knob::tile_order_sort();
        const uint64_t NRa = (uint64_t)NR + 1;
        auto *d_recoff = pool.take<unsigned long long>(NRa);
        auto *d_recsample = pool.take<uint16_t>(NRa);
        auto *d_rd = pool.take<uint4>(NRa);
        auto *d_pre = pool.take<RecCnt>(NRa);
        auto *d_ftile = pool.take<uint32_t>(NRa);
        auto *d_flags = pool.take<uint8_t>(NRa);
        auto *d_rg = pool.take<unsigned long long>(NRa);
        if (int rc = take_run_group_tables()) return rc;
        if (int rc = alloc_round_buffers()) return rc;
        TB = RdTables{d_recoff, d_recsample, d_recbase, d_rd, d_pre, d_ftile, d_flags, d_rg, d_runfirst, d_grpfirst};
        if (n_sub) hipLaunchKernelGGL(msnv_scan_write2, grid_for(n_sub, 256), dim3(256), 0, st, W.d_ss, (uint32_t)S, n_sub, sub_bytes, cap2, W.d_cnt, d_subbase, d_bflag, W.d_delta, d_slots, d_info, TB, d_acc, d_misc,
                                      d_outl, span_out, T.overhang, P);
        HIP_TRY(hipGetLastError());
        totals_h = RecCnt{tot.pile, tot.npiece, tot.niv, tot.spill, tot.seqb};
        HIP_TRY(hipMemcpyAsync(d_pre + NR, &totals_h, sizeof(RecCnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_recoff + NR, &end_all, 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_recbase + S, &NR, 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(msnv_group_pre2, grid_for((uint64_t)n_groups + 1, 256), dim3(256), 0, st, n_groups, NR, d_grpfirst, TB.r_pre, d_grppre);
        hipLaunchKernelGGL(msnv_acc_fold, dim3((unsigned)S), dim3(64), 0, st, d_acc, (uint32_t)S);
        HIP_TRY(hipGetLastError());
        // ---- the depth stage on the context's SECOND stream, beside the layout and the emit kernels on the first (round 6: msnv_depth2
        // writes the pieces' depths itself, so nothing the emit kernels read comes from it); what the host needs of it goes to the pinned
        // words behind it, with an event (evd2)
        if (!ds.ctx->stream2) { if (int rc = dev_stream_create(&ds.ctx->stream2)) return rc; }
        const bool depth_on_main = knob::depth_on_main();      // (A/B: the depth stage in front of the emit kernels, on their stream)
        hipStream_t st2 = depth_on_main ? st : (hipStream_t)ds.ctx->stream2;
        HIP_TRY(hipEventRecord((hipEvent_t)T.pending.evw, st));
        HIP_TRY(hipStreamWaitEvent(st2, (hipEvent_t)T.pending.evw, 0));
        HIP_TRY(hipEventRecord((hipEvent_t)T.pending.evd, st2)); T.pending.has_evd = true;
        return launch_depth_stage(st2);
    }

    // ================================================================ CAREFUL: stage by stage
    // Takes: the staged streams.  Leaves: what front_quick() leaves, everything waited for and looked at (errors reported), and what
    // edit_qualities() needs: the overlapping mates' groups (o_*), the samples of the kernels' edits (dev_tok), the host pre-pass's verdicts
    // (d_ovr, cut_marks, host_sample).  Two passes at the most: the second measures again behind the pre-pass and msnv_cap_reads.
    int front_careful() {
        if (int rc = begin_route(false)) return rc;
        SR.ms_scan = 0; SR.n_redone = 0;
        if (int rc = scan_records(st, pool, n_bytes, S, NC, SR)) return rc;
        T.ms_scan += SR.ms_scan; T.n_scan_redone += SR.n_redone;
        NR = SR.NR;
        const uint64_t NRa = (uint64_t)NR + 1, NBa = ((uint64_t)NR + PB - 1) / PB + 1;   // blocks of PB records: their sums and bases (entry NB of the bases = the round's totals)
        d_recbase = SR.d_recbase; d_send = SR.d_send;
        fin_trace("  pack: scan done");
        c_flags0 = pool.take<uint8_t>(NRa);
        c_key = pool.take<unsigned long long>(NRa);
        c_end = pool.take<uint32_t>(NRa);
        c_maxc = pool.take<uint32_t>(NRa);
        auto *d_ftile = pool.take<uint32_t>(NRa);
        c_cnt = pool.take<RecCnt>(NRa);
        c_blkcnt = pool.take<RecCnt>(NBa);
        c_blkpre = pool.take<RecCnt>(NBa);
        d_ovr = pool.take<uint32_t>(NRa);
        auto *d_rd = pool.take<uint4>(NRa);
        auto *d_pre = pool.take<RecCnt>(NRa);
        auto *d_flags = pool.take<uint8_t>(NRa);
        auto *d_rg = pool.take<unsigned long long>(NRa);
        c_sf = pool.take<unsigned long long>(NRa);
        d_depth0 = pool.take<uint32_t>(NRa);
        d_hot = pool.take<uint32_t>(NRa);
        d_hotn = pool.take<uint32_t>(2);
        if (pool.rc) return pool.rc;
        d_capfail = d_hotn + 1;
        HIP_TRY(hipMemsetAsync(d_hotn, 0, 8, st));
        TB = RdTables{SR.d_recoff, SR.d_recsample, d_recbase, d_rd, d_pre, d_ftile, d_flags, d_rg, nullptr, nullptr};
        HIP_TRY(hipMemcpyAsync(SR.d_recoff + NR, &end_all, 8, hipMemcpyHostToDevice, st));
        const size_t depth_bufs_from = pool.mark();
        for (int pass = 0; pass < 2; ++pass) {
            pool.rewind(depth_bufs_from);
            if (int rc = measure()) return rc;
            if (int rc = tables_and_depth()) return rc;
            const bool ovl_on_host = knob::overlap_on_host();      // (read per pass, like MSNV_PREPASS below: the tests switch them)
            if (int rc = list_overlaps(pass, ovl_on_host)) return rc;
            if (pass == 1) {
                if (!dev_cap.empty()) {
                    uint32_t cap_fail = 0;
                    HIP_TRY(hipMemcpy(&cap_fail, d_capfail, 4, hipMemcpyDeviceToHost));
                    if (cap_fail) return fail(MSNV_EINVAL, "internal: the depth-cap kernel met a read that spans more than its ring holds");
                }
                break;
            }
            bool second_pass = false;
            if (int rc = sequential_edits(ovl_on_host, second_pass)) return rc;
            if (!second_pass) break;
        }
        return MSNV_OK;
    }
    // msnv_measure_reads and the scan of its blocks' sums; again with a wider window when more far-reaching reads turn up than the list holds.
    // Leaves: the round's totals (tot_c, NPC, NIV, seqb_total), misc_h.  One wait per turn.
    int measure() {
        const uint64_t NB = ((uint64_t)NR + PB - 1) / PB;
        hipLaunchKernelGGL(msnv_acc_init, grid_for(S * ACC_COPIES, 256), dim3(256), 0, st, d_acc, (uint32_t)(S * ACC_COPIES));
        HIP_TRY(hipGetLastError());
        tm.start();
        for (;;) {
            HIP_TRY(hipMemsetAsync(d_misc, 0, MISC_WORDS * 4, st));
            HIP_TRY(hipMemsetAsync(c_blkcnt + NB, 0, sizeof(RecCnt), st));
            if (NR) {
                hipLaunchKernelGGL(msnv_measure_reads, grid_for(NR, 256), dim3(256), 0, st, raw, TB.rec_off, TB.rec_sample, d_recbase, d_send, NR, ctg, P, have_ovr ? d_ovr : nullptr, c_flags0,
                                   c_key, c_end, c_maxc, c_cnt, TB.r_ftile, c_blkcnt, d_acc, d_misc, d_outl, span_out, T.overhang);
                HIP_TRY(hipGetLastError());
            }
            // every block's base: rank among the pileup reads, first piece, first interval, next-tile pieces before it, first seq byte
            if (int rc = prim.exclusive(c_blkcnt, c_blkpre, RecCnt{}, (size_t)(NB + 1), RecCntSum())) return rc;
            HIP_TRY(hipMemcpyAsync(&tot_c, c_blkpre + NB, sizeof(RecCnt), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(misc_h, d_misc, MISC_WORDS * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (misc_h[MISC_NOUT] <= CAP_OUT || span_out >= 0x40000000u) break;
            // more far-reaching reads than the list holds (long reads): they are the ordinary reads of this round -- a wider window, again
            span_out = span_out < 0x04000000u ? span_out * 16u : 0x7fffffffu;
            hipLaunchKernelGGL(msnv_acc_init, grid_for(S * ACC_COPIES, 256), dim3(256), 0, st, d_acc, (uint32_t)(S * ACC_COPIES));
            HIP_TRY(hipGetLastError());
        }
        T.ms_measure += tm.stop();
        fin_trace("  pack: measure + block scan (sync)");
        NPC = tot_c.npiece; NIV = tot_c.niv; seqb_total = tot_c.seqb;
        return MSNV_OK;
    }
    // The records' tables in the quick route's form (run and group numbers by a scan of their start flags), the round's buffers, the depth
    // stage -- on the round's own stream, waited for; then the errors.  Leaves: TB filled, runs / groups / acc / misc_h on the host.
    int tables_and_depth() {
        tm.start();
        n_runs = 0; n_groups = 0;
        if (NR) {
            hipLaunchKernelGGL(msnv_tables_from_measure, grid_for(NR, 256), dim3(256), 0, st, NR, TB.rec_sample, c_flags0, c_key, c_end, c_maxc, c_cnt, c_blkpre, TB.r_ftile, span_out, P, TB, c_sf, d_acc, d_misc);
            HIP_TRY(hipGetLastError());
            if (int rc = prim.inclusive(c_sf, TB.r_rg, (size_t)NR, rocprim::plus<unsigned long long>())) return rc;
            unsigned long long last = 0;
            HIP_TRY(hipMemcpyAsync(&last, TB.r_rg + (NR - 1), 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(misc_h, d_misc, MISC_WORDS * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            n_runs = (uint32_t)(last >> 32); n_groups = (uint32_t)last;
        }
        in_order = misc_h[MISC_SORT] != 0 || knob::tile_order_sort();      // (the tile order's route: the depth kernel writes the pieces' depths at their header slots)
        totals_h = tot_c;
        HIP_TRY(hipMemcpyAsync(TB.r_pre + NR, &totals_h, sizeof(RecCnt), hipMemcpyHostToDevice, st));
        if (int rc = take_run_group_tables()) return rc;
        if (int rc = alloc_round_buffers()) return rc;
        // (the groups' first records: this route has no table of them yet -- the depth kernel writes it, the places follow, then the depths)
        hipLaunchKernelGGL(msnv_group_firsts, grid_for(NR, 256), dim3(256), 0, st, NR, TB.r_flags, TB.r_rg, d_runfirst, d_grpfirst);
        hipLaunchKernelGGL(msnv_group_pre2, grid_for((uint64_t)n_groups + 1, 256), dim3(256), 0, st, n_groups, NR, d_grpfirst, TB.r_pre, d_grppre);
        HIP_TRY(hipGetLastError());
        if (int rc = launch_depth_stage(st)) return rc;
        hipLaunchKernelGGL(msnv_acc_fold, dim3((unsigned)S), dim3(64), 0, st, d_acc, (uint32_t)S);
        HIP_TRY(hipGetLastError());
        runs.resize(n_runs); groups.resize(n_groups);
        HIP_TRY(hipMemcpyAsync(runs.data(), d_runs, (size_t)n_runs * sizeof(DpRun), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(groups.data(), d_groups, (size_t)n_groups * sizeof(DevGroupRec), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpy2DAsync(acc.data(), sizeof(DpAcc), d_acc, sizeof(DpAcc) * ACC_COPIES, sizeof(DpAcc), S, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(misc_h, d_misc, MISC_WORDS * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        T.ms_depth += tm.stop();
        fin_trace("  pack: depth stage (sync)");
        rec_base_h = SR.rec_base;
        return check_errors();
    }
    // ---- overlapping mates: the candidates grouped by (sample, name); nothing is edited yet (MSNV_OVERLAP=host: the host pre-pass does it).
    // The second pass lists them again when msnv_cap_reads has taken reads out: a dropped read is no candidate (sam.c overlap_remove).
    // Leaves: n_ovl_reads, n_ovl_groups, o_starts / o_svals (the groups), o_skip; need_host of samples whose templates overflow the slots.
    int list_overlaps(int pass, bool ovl_on_host) {
        const uint64_t NRa = (uint64_t)NR + 1;
        bool any_ovl = false;
        for (size_t s = 0; s < S; ++s) any_ovl |= !MP.ignore_overlaps && acc[s].n_ovl >= 2;
        if (pass == 1 && !dev_cap.empty()) { n_ovl_reads = 0; n_ovl_groups = 0; }
        if (!any_ovl || ovl_on_host || (pass == 1 && dev_cap.empty())) return MSNV_OK;
        tm.start();
        if (int rc = o_flag.alloc(NRa * 4)) return rc;
        if (int rc = o_rank.alloc(NRa * 4)) return rc;
        if (int rc = o_skip.alloc(S)) return rc;
        HIP_TRY(hipMemsetAsync(o_skip.p, 0, S, st));
        hipLaunchKernelGGL(msnv_ovl_mark, grid_for(NRa, 256), dim3(256), 0, st, TB.r_flags, NR, TB.rec_sample, o_skip.as<uint8_t>(), o_flag.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        if (int rc = prim.scan32(o_flag.as<uint32_t>(), o_rank.as<uint32_t>(), NRa, false)) return rc;
        HIP_TRY(hipMemcpyAsync(&n_ovl_reads, o_rank.as<uint32_t>() + NR, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_ovl_reads >= 2) {
            const uint64_t NOa = (uint64_t)n_ovl_reads + 1;
            if (int rc = o_keys.alloc(NOa * 8)) return rc;
            if (int rc = o_skeys.alloc(NOa * 8)) return rc;
            if (int rc = o_vals.alloc(NOa * 4)) return rc;
            if (int rc = o_svals.alloc(NOa * 4)) return rc;
            hipLaunchKernelGGL(msnv_ovl_list, grid_for(NR, 256), dim3(256), 0, st, TB.r_flags, o_rank.as<uint32_t>(), NR, raw, TB.rec_off, TB.rec_sample, o_skip.as<uint8_t>(),
                               o_keys.as<unsigned long long>(), o_vals.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            if (int rc = prim.sort64(o_keys.as<unsigned long long>(), o_skeys.as<unsigned long long>(), o_vals.as<uint32_t>(), o_svals.as<uint32_t>(), n_ovl_reads, 64u)) return rc;
            // groups of equal keys: flags and their scan in the unsorted arrays' memory
            uint32_t *gflag = o_vals.as<uint32_t>(), *gid = reinterpret_cast<uint32_t *>(o_keys.p);
            hipLaunchKernelGGL(msnv_pair_flags, grid_for(n_ovl_reads, 256), dim3(256), 0, st, o_skeys.as<unsigned long long>(), n_ovl_reads, gflag);
            HIP_TRY(hipGetLastError());
            if (int rc = prim.scan32(gflag, gid, n_ovl_reads, true)) return rc;
            HIP_TRY(hipMemcpyAsync(&n_ovl_groups, gid + (n_ovl_reads - 1), 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = o_starts.alloc(((uint64_t)n_ovl_groups + 1) * 4)) return rc;
            hipLaunchKernelGGL(msnv_ovl_group_starts, grid_for(n_ovl_reads, 256), dim3(256), 0, st, gflag, gid, n_ovl_reads, o_starts.as<uint32_t>());
            hipLaunchKernelGGL(msnv_ovl_check, grid_for(n_ovl_groups, 256), dim3(256), 0, st, o_starts.as<uint32_t>(), n_ovl_groups, n_ovl_reads, o_svals.as<uint32_t>(), TB.rec_sample, d_acc);
            HIP_TRY(hipGetLastError());
            std::vector<DpAcc> again(S);
            HIP_TRY(hipMemcpy2DAsync(again.data(), sizeof(DpAcc), d_acc, sizeof(DpAcc) * ACC_COPIES, sizeof(DpAcc), S, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t s = 0; s < S; ++s) acc[s].need_host = again[s].need_host;
        }
        T.ms_depth += tm.stop();
        return MSNV_OK;
    }
    // ---- which samples need the sequential edits?  The depth cap and the token limit are kernels (msnv_cap_reads, msnv_token_cut; round 6);
    // the host pre-pass keeps what they do not take: a template with more alignments than the overlap kernel's slots, an element longer
    // than the tables can say, a round with far-reaching reads (the cap kernel's ring, the token kernel's window) -- and MSNV_PREPASS=host.
    // Leaves: dev_cap, dev_tok, host_sample; `second_pass` when a verdict changes who enters the pileup (d_ovr then holds the verdicts).
    int sequential_edits(bool ovl_on_host, bool &second_pass) {
        const bool prepass_on_host = knob::prepass_on_host();      // (read per round: the tests switch it)
        const bool kernels_can = !prepass_on_host && misc_h[MISC_NOUT] == 0u && span_out == SPAN_OUT && misc_h[MISC_SPAN] <= CAP_RING;
        std::vector<size_t> need;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t nh = acc[s].need_host;
            if ((nh & (NEED_OVL | NEED_BIGC)) || (nh && !kernels_can) || (ovl_on_host && !MP.ignore_overlaps && acc[s].n_ovl >= 2)) need.push_back(s);
            else {
                if (nh & NEED_CAP) dev_cap.push_back((uint32_t)s);
                if (nh & NEED_TOKEN) dev_tok.push_back((uint32_t)s);
            }
        }
        for (size_t s : need) host_sample[s] = 1;
        T.n_device_edit_samples += dev_tok.size();
        for (uint32_t s : dev_cap) if (!(acc[s].need_host & NEED_TOKEN)) T.n_device_edit_samples += 1;
        second_pass = !need.empty() || !dev_cap.empty();           // (the token limit alone: the reads msnv_depth2 has listed stand)
        if (!second_pass) return MSNV_OK;
        if (int rc = host_prepass_samples(need)) return rc;
        if (!dev_cap.empty()) {                                    // who enters the pileup of these samples: a wavefront each (into d_ovr, behind the host's verdicts)
            auto *d_caplist = pool.take<uint32_t>(dev_cap.size());
            if (pool.rc) return pool.rc;
            HIP_TRY(hipMemcpyAsync(d_caplist, dev_cap.data(), dev_cap.size() * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(msnv_cap_reads, dim3((unsigned)dev_cap.size()), dim3(64), 0, st, d_caplist, d_recbase, TB.rd, TB.r_flags, d_depth0, MP.max_depth, d_ovr, d_capfail);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));                     // (dev_cap's bytes; the second pass takes the pool's buffers back)
        }
        return MSNV_OK;
    }
    // pack.cpp: host_prepass over the samples of `need`, on host threads; its verdicts per record go up into d_ovr (zeros for everyone else),
    // the records it patched back into the streams.  Blocking copies only.
    int host_prepass_samples(const std::vector<size_t> &need) {
        const double t0 = now_s();
        T.n_prepass_samples += need.size();
        std::vector<uint32_t> ovr_all((size_t)NR + 1, 0u);
        std::vector<std::vector<uint8_t>> host_copy(need.size()), patched(need.size());
        std::vector<int> rcs(need.size(), 0); std::vector<std::string> msgs(need.size());
        for (size_t k = 0; k < need.size(); ++k) if (on_device) {
            host_copy[k].resize(n_bytes[need[k]]);
            if (n_bytes[need[k]]) HIP_TRY(hipMemcpy(host_copy[k].data(), raw + SR.s_beg[need[k]], n_bytes[need[k]], hipMemcpyDeviceToHost));
        }
        {
            std::atomic<size_t> next{0};
            auto w = [&]() {
                for (;;) {
                    const size_t k = next.fetch_add(1);
                    if (k >= need.size()) break;
                    const size_t s = need[k];
                    const uint8_t *rec = on_device ? host_copy[k].data() : streams[s];
                    std::vector<uint32_t> ov; bool cm = false;
                    int rc;
                    try { rc = host_prepass(ds, rec, n_bytes[s], ov, patched[k], cm); } catch (const std::exception &e) { rc = fail_quiet(MSNV_ENOMEM, "host pre-pass: %s", e.what()); }
                    if (!rc && ov.size() != SR.n_rec[s]) rc = fail_quiet(MSNV_EINVAL, "internal: the host pre-pass saw %zu records, the device scan %u", ov.size(), SR.n_rec[s]);
                    if (rc) { rcs[k] = rc; msgs[k] = msnv_last_error(); continue; }
                    std::copy(ov.begin(), ov.end(), ovr_all.begin() + SR.rec_base[s]);
                    cut_marks[s] = cm ? 1 : 0;
                }
            };
            std::vector<std::thread> th;
            const size_t nt = std::min<size_t>(need.size(), msnv_default_threads());
            for (size_t k = 0; k < nt; ++k) th.emplace_back(w);
            for (auto &x : th) x.join();
        }
        for (size_t k = 0; k < need.size(); ++k) if (rcs[k]) return fail(rcs[k], "%s", msgs[k].c_str());
        for (size_t k = 0; k < need.size(); ++k) if (!patched[k].empty()) HIP_TRY(hipMemcpy(raw + SR.s_beg[need[k]], patched[k].data(), patched[k].size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_ovr, ovr_all.data(), ((uint64_t)NR + 1) * 4, hipMemcpyHostToDevice));
        have_ovr = true;
        if (!need.empty()) T.wall_prepass_s += now_s() - t0;
        return MSNV_OK;
    }

    // Takes: the careful front's groups and lists.  Leaves: the qualities of overlapping mates edited where they lie (msnv_ovl_groups), then
    // snpCall's token limit: the bases behind the cut get their mark (behind the mates' edits: the -Q test sees them).
    int edit_qualities() {
        if (n_ovl_groups) {
            tm.start();
            HIP_TRY(hipMemcpyAsync(o_skip.p, host_sample.data(), S, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(msnv_ovl_groups, grid_for(n_ovl_groups, 64), dim3(64), 0, st, o_starts.as<uint32_t>(), n_ovl_groups, n_ovl_reads, o_svals.as<uint32_t>(), raw, TB.rec_off, TB.rd,
                               TB.rec_sample, o_skip.as<uint8_t>());
            HIP_TRY(hipGetLastError());
            T.ms_depth += tm.stop();
        }
        if (!dev_tok.empty()) {
            tm.start();
            std::vector<uint8_t> tk(S, 0);
            for (uint32_t s : dev_tok) { tk[s] = 1; cut_marks[s] = 1; }
            auto *d_tok = pool.take<uint8_t>(S);
            if (pool.rc) return pool.rc;
            HIP_TRY(hipMemcpyAsync(d_tok, tk.data(), S, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(msnv_token_clamp, grid_for((uint64_t)NR * 64u, 256), dim3(256), 0, st, d_tok, TB.rec_sample, TB.r_flags, NR, raw, TB.rec_off);
            hipLaunchKernelGGL(msnv_token_cut, dim3(4096), dim3(256), 0, st, d_hot, d_hotn, d_tok, d_recbase, TB.rd, TB.r_flags, raw, TB.rec_off, d_misc + MISC_SPAN, P);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));                             // (tk's bytes)
            T.ms_depth += tm.stop();
        }
        fin_trace("  pack: checks, overlaps");
        return MSNV_OK;
    }

    // ================================================================ layout + emit (both routes)
    // Takes: a front's tables and buffers.  Leaves: msnv_sample_layout, the emit kernels and the fold RUNNING (T.pending), and on their way
    // into the dataset's pinned words what the host needs of the stages so far, with an event behind the copies (evh; the quick route's depth
    // stage: evd2).  The emit kernels are launched first, THEN collect() waits for the events.  Does not wait (but for the FASTA thread).
    int launch_emit() {
        const uint64_t NB = ((uint64_t)NR + PB - 1) / PB;
        HIP_TRY(hipMemcpyAsync(d_cut, cut_marks.data(), S, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_slow, 0, 4, st));
        hipLaunchKernelGGL(msnv_sample_layout, dim3(1), dim3(256), 0, st, d_recbase, (uint32_t)S, TB.r_pre, d_acc, TB.rd, r_seq, r_qual, d_cut, d_sum, d_ss0, d_dst, d_pb);
        HIP_TRY(hipGetLastError());
        const uint64_t b_acc = S * sizeof(DpAcc), b_sum = (S + 1) * sizeof(DpSampleSum2), b_pb = S * 8, b_rb = (S + 1) * 4, b_runs = (uint64_t)n_runs * sizeof(DpRun), b_grp = (uint64_t)n_groups * sizeof(DevGroupRec);
        auto up8 = [](uint64_t v) { return (v + 15) & ~15ull; };
        o_acc = up8(((uint64_t)ds.samples.size() + 16) * 4); o_sum = o_acc + up8(b_acc); o_pb = o_sum + up8(b_sum); o_rb = o_pb + up8(b_pb); o_misc = o_rb + up8(b_rb); o_runs = o_misc + 16; o_grp = o_runs + up8(b_runs);
        const uint64_t o_end = o_grp + up8(b_grp);
        if (int rc = pin_ensure(ds, std::max<uint64_t>(o_end, S * sizeof(DpAcc) + 16))) return rc;      // (+ 16: the emit kernels' count of slow blocks behind the accumulators)
        pinb = static_cast<uint8_t *>(T.pin) + T.pin_cap / 2;
        if (quick) {
            const bool depth_on_main = knob::depth_on_main();
            hipStream_t st2 = depth_on_main ? st : (hipStream_t)ds.ctx->stream2;          // (behind the depth stage: its stream)
            HIP_TRY(hipMemcpy2DAsync(pinb + o_acc, sizeof(DpAcc), d_acc, sizeof(DpAcc) * ACC_COPIES, sizeof(DpAcc), S, hipMemcpyDeviceToHost, st2));
            HIP_TRY(hipMemcpyAsync(pinb + o_rb, d_recbase, b_rb, hipMemcpyDeviceToHost, st2));
            HIP_TRY(hipMemcpyAsync(pinb + o_misc, d_misc, MISC_WORDS * 4, hipMemcpyDeviceToHost, st2));
            if (n_runs) HIP_TRY(hipMemcpyAsync(pinb + o_runs, d_runs, b_runs, hipMemcpyDeviceToHost, st2));
            if (n_groups) HIP_TRY(hipMemcpyAsync(pinb + o_grp, d_groups, b_grp, hipMemcpyDeviceToHost, st2));
            HIP_TRY(hipEventRecord((hipEvent_t)T.pending.evd2, st2));
        }
        HIP_TRY(hipMemcpyAsync(pinb + o_sum, d_sum, b_sum, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pinb + o_pb, d_pb, b_pb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord((hipEvent_t)T.pending.evh, st));
        if (int rc = tables.join()) return rc;                        // (the packed FASTA: the emit kernels read it)
        HIP_TRY(hipEventRecord((hipEvent_t)T.pending.ev0, st));
        if (NR) {
            EmitArgs A{};
            A.raw = raw; A.rec_off = TB.rec_off; A.rec_sample = TB.rec_sample; A.n_rec = NR; A.ctg = ctg; A.r_flags = TB.r_flags; A.r_pre = TB.r_pre;
            A.samp_sbase0 = d_ss0; A.rg = TB.r_rg; A.grp_pre = d_grppre; A.in_order = in_order ? 1u : 0u;
            A.hdr = w_hdr; A.ptid = w_tid; A.pend = w_end; A.cov_tid = keep.cov_tid; A.cov_beg = keep.cov_beg; A.cov_end = keep.cov_end;
            A.noseq_counts = (P.c_eff == 0 && !P.all_low) ? 1u : 0u;
            A.pref4 = T.pref4; A.P = P; A.dst = d_dst; A.acc = d_acc;
            A.slow = d_slow; A.force_slow = knob::emit_slow() ? 1u : 0u;
            const bool dbg = knob::debug_sync();
            if (dbg) { HIP_TRY(hipStreamSynchronize(st)); fin_trace("  dbg: before emit"); }
            hipLaunchKernelGGL(msnv_emit_block, dim3((unsigned)NB), dim3(256), 0, st, A);
            if (dbg) { HIP_TRY(hipStreamSynchronize(st)); fin_trace("  dbg: emit_block"); }
            hipLaunchKernelGGL(msnv_emit_block_slow, dim3((unsigned)std::min<uint64_t>(NB, 2048)), dim3(256), 0, st, A);
            if (dbg) { HIP_TRY(hipStreamSynchronize(st)); fin_trace("  dbg: emit_block_slow"); }
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(msnv_emit_tail, dim3((unsigned)S), dim3(64), 0, st, d_dst, d_pb, (uint32_t)S, P);
        if (knob::debug_sync()) { HIP_TRY(hipStreamSynchronize(st)); fin_trace("  dbg: emit_tail"); }
        if (quick) HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)T.pending.evd2, 0));      // (the depth stage's last words into the accumulators: in front of their fold)
        hipLaunchKernelGGL(msnv_acc_fold, dim3((unsigned)S), dim3(64), 0, st, d_acc, (uint32_t)S);
        HIP_TRY(hipGetLastError());
        // The round's last kernels are left RUNNING: nothing the host still has to do for this round -- its (sample, tile) pairs, its tables --
        // and little of what finalize does first needs the bases or the headers.  What they leave for the host (the mismatch sample of every
        // sample, their time) comes through pinned memory and is taken by devpack_sync_pending.
        HIP_TRY(hipMemcpy2DAsync(T.pin, sizeof(DpAcc), d_acc, sizeof(DpAcc) * ACC_COPIES, sizeof(DpAcc), S, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(static_cast<uint8_t *>(T.pin) + S * sizeof(DpAcc), d_slow, 4, hipMemcpyDeviceToHost, st));      // (how many blocks msnv_emit_block left to msnv_emit_block_slow: same event, no wait of its own)
        HIP_TRY(hipEventRecord((hipEvent_t)T.pending.ev1, st));
        T.pending.active = true; T.pending.first = first; T.pending.n = S;
        return MSNV_OK;
    }

    // the round is not to be: nothing stays pending, and its kernels have run before anyone frees what they write into
    int withdraw() { T.pending.active = false; HIP_TRY(hipStreamSynchronize(st)); return MSNV_OK; }

    // ---- the host's share.  Takes: the pinned words.  Waits for the small results (evh, evd2), not for the emit kernels, and looks at them.
    // Leaves: sum, piece_bytes (quick: acc, rec_base_h, misc_h, runs, groups too) on the host; the round's buffers the dataset's.  Or
    // TO_CAREFUL (quick route only): the round withdrawn, `held` still holding its buffers for the next route to drop.
    int collect() {
        HIP_TRY(hipEventSynchronize((hipEvent_t)T.pending.evh));
        if (quick) HIP_TRY(hipEventSynchronize((hipEvent_t)T.pending.evd2));
        fin_trace("  pack: depth stage, layout (wait)");
        memcpy(sum.data(), pinb + o_sum, (S + 1) * sizeof(DpSampleSum2));
        memcpy(piece_bytes.data(), pinb + o_pb, S * 8);
        if (quick) {
            memcpy(acc.data(), pinb + o_acc, S * sizeof(DpAcc));
            rec_base_h.assign(S + 1, 0); memcpy(rec_base_h.data(), pinb + o_rb, (S + 1) * 4);
            memcpy(misc_h, pinb + o_misc, MISC_WORDS * 4);
            runs.resize(n_runs); groups.resize(n_groups);
            if (n_runs) memcpy(runs.data(), pinb + o_runs, (size_t)n_runs * sizeof(DpRun));
            if (n_groups) memcpy(groups.data(), pinb + o_grp, (size_t)n_groups * sizeof(DevGroupRec));
            // what the quick route could not know when it launched the emit kernels: an error (reported), or something only the careful route
            // handles -- a sample that needs the host pre-pass (depth cap, token limit), more far-reaching reads than the list holds, two
            // overhanging contigs in one sub-segment.  The round is taken back (the kernels that still write into its buffers are waited for)
            bool again = misc_h[MISC_NOUT] > CAP_OUT || misc_h[MISC_OVERHANG] == 2u;
            for (size_t s = 0; s < S; ++s) again |= acc[s].need_host != 0;
            const int rc_err = check_errors();
            if (rc_err || again) {
                if (int rc = withdraw()) return rc;
                if (rc_err) return rc_err;
                T.n_quick_redone += 1;
                return TO_CAREFUL;
            }
        }
        if (misc_h[MISC_OVERHANG]) T.any_overhang_h = true;
        for (size_t s = 0; s < S; ++s)
            if (piece_bytes[s] > 0xffffff00ull) { if (int rc = withdraw()) return rc; return fail(MSNV_EDOMAIN, "one sample holds more than 8.5 G aligned bases in this shard: shard the contigs further"); }
        keep.seq_total = sum[S].seq_off;
        T.n_pieces += NPC; T.n_records += NR;
        T.pad_in_emit = true;                                          // (msnv_emit_block* leave the alignment nibbles behind every piece as finalize wants them)
        T.round_bufs.push_back(held.round_buf); held.round_buf = nullptr;
        held.keep_buf = nullptr;                                       // (the dataset's from here on)
        T.rounds.push_back(keep);
        if (in_order) {                                                // (the general tile-order route of tile_pairs() waits for its sort anyway)
            if (int rc = devpack_sync_pending(ds)) return rc;
            // (the round's samples are not the dataset's yet: publish() takes the mismatch sample from `acc`, so the emit kernels' counts go there)
            const DpAcc *a = static_cast<const DpAcc *>(T.pin);
            for (size_t s = 0; s < S; ++s) { acc[s].mm_bases = a[s].mm_bases; acc[s].mm = a[s].mm; }
        }
        fin_trace("  pack: emit launched, results in");
        return MSNV_OK;
    }

    // ---- the (sample, contig, tile) runs of pieces = the pairs of the tile index.  Takes: the headers (in_order: work buffers, emitted) or the
    // groups on the host.  Leaves: `prec` -- the sort route's still on its way down (publish() waits), the headers in tile order in `keep`.
    int tile_pairs() {
        if (in_order) tm.start();
        if (NPC >= 1 && in_order) {
            // the general route: stable sort of the headers by (sample, contig, tile), runs of equal keys
            const uint64_t NPCa = (uint64_t)NPC + 1;
            auto *d_tk = pool.take<unsigned long long>(NPCa);
            auto *d_ix = pool.take<uint32_t>(NPCa);
            auto *d_uns = pool.take<uint32_t>(4);
            if (pool.rc) return pool.rc;
            HIP_TRY(hipMemsetAsync(d_uns, 0, 4, st));
            const unsigned tid_bits = std::max(1u, bit_width_u64(NC ? NC - 1 : 0));
            hipLaunchKernelGGL(msnv_tile_keys, grid_for(NPC, 256), dim3(256), 0, st, w_hdr, w_tid, d_dst, (uint32_t)S, NPC, tid_bits, d_tk, d_ix, d_uns);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&uns_h, d_uns, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const unsigned long long *skeys = d_tk;
            auto *d_tk2 = pool.take<unsigned long long>(NPCa);
            auto *d_ix2 = pool.take<uint32_t>(NPCa);
            if (pool.rc) return pool.rc;
            if (uns_h) {
                if (int rc = prim.sort64(d_tk, d_tk2, d_ix, d_ix2, NPC, 21u + tid_bits + std::max(1u, bit_width_u64(S - 1)))) return rc;
                hipLaunchKernelGGL(msnv_gather_pieces, grid_for(NPC, 256), dim3(256), 0, st, d_ix2, NPC, w_hdr, w_tid, w_end, w_depth, keep.hdr, keep.tid, keep.end, keep.depth);
                HIP_TRY(hipGetLastError());
                skeys = d_tk2;
            } else {
                HIP_TRY(hipMemcpyAsync(keep.hdr, w_hdr, (size_t)NPC * sizeof(ReadHdr), hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(keep.tid, w_tid, (size_t)NPC * 4, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(keep.end, w_end, (size_t)NPC * 4, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(keep.depth, w_depth, (size_t)NPC * 2, hipMemcpyDeviceToDevice, st));
            }
            // runs of equal keys (d_ix / d_ix2 are free again: flags and their scan)
            hipLaunchKernelGGL(msnv_pair_flags, grid_for(NPC, 256), dim3(256), 0, st, skeys, NPC, d_ix);
            HIP_TRY(hipGetLastError());
            if (int rc = prim.scan32(d_ix, d_ix2, NPC, true)) return rc;
            HIP_TRY(hipMemcpyAsync(&n_pairs_h, d_ix2 + (NPC - 1), 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint32_t n_pairs = n_pairs_h;
            auto *d_prec = pool.take<DevPairRec>((uint64_t)n_pairs + 1);
            if (pool.rc) return pool.rc;
            hipLaunchKernelGGL(msnv_pair_starts, grid_for(NPC, 256), dim3(256), 0, st, skeys, d_ix, d_ix2, NPC, tid_bits, d_prec);
            hipLaunchKernelGGL(msnv_pair_maxd, grid_for(n_pairs, 64), dim3(64), 0, st, d_prec, n_pairs, NPC, keep.depth);
            HIP_TRY(hipGetLastError());
            prec.resize(n_pairs);
            HIP_TRY(hipMemcpyAsync(prec.data(), d_prec, (size_t)n_pairs * sizeof(DevPairRec), hipMemcpyDeviceToHost, st));
        } else if (NPC >= 1) {
            // tile order by counting: a group's pieces in its own tile join the ones the group before leaves there (same contig, the tile before)
            prec.reserve(groups.size() + groups.size() / 8);
            for (size_t g = 0; g < groups.size(); ++g) {
                const DevGroupRec &G = groups[g];
                const bool prev_adj = g > 0 && groups[g - 1].sample == G.sample && groups[g - 1].tid == G.tid && groups[g - 1].tile + 1u == G.tile;
                const bool next_adj = g + 1 < groups.size() && groups[g + 1].sample == G.sample && groups[g + 1].tid == G.tid && groups[g + 1].tile == G.tile + 1u;
                prec.push_back(DevPairRec{G.sample, G.tid, G.tile, prev_adj ? groups[g - 1].b : G.a, std::max(G.md_own, prev_adj ? groups[g - 1].md_next : 0u)});
                if (!next_adj && G.end > G.b) prec.push_back(DevPairRec{G.sample, G.tid, G.tile + 1u, G.b, G.md_next});
            }
        }
        if (in_order) T.ms_sort += tm.stop();                          // (the counting route is host work on the groups: nothing to wait for)
        fin_trace("  pack: pairs");
        return MSNV_OK;
    }

    // ---- what the host keeps of a sample: its summaries and its (contig, tile) runs.  Takes: acc, sum, piece_bytes, prec, runs.
    int publish() {
        const double t_dl = now_s();
        const int32_t round_no = (int32_t)T.rounds.size() - 1;
        for (size_t s = 0; s < S; ++s) {
            SampleCols &sc = ds.samples[first + s];
            const DpAcc &a = acc[s];
            sc.on_device = true; sc.d_seq = r_seq + sum[s].seq_off; sc.d_qual = r_qual + sum[s].seq_off / 4; sc.d_seq_bytes = piece_bytes[s] + 32;
            sc.dev_index = true; sc.dev_round = round_no; sc.dev_piece0 = sum[s].pbase0; sc.dev_iv0 = sum[s].ibase0;
            sc.n_dev_pieces = sum[s + 1].pbase0 - sum[s].pbase0; sc.n_dev_iv = sum[s + 1].ibase0 - sum[s].ibase0;
            sc.n_pileup_bases = a.n_bases; sc.n_pileup_reads = a.n_pile_reads;
            sc.mm_sampled_bases = a.mm_bases; sc.mm_sampled = a.mm;
            sc.alg_seq_bytes = a.alg_seq; sc.alg_qual_bytes = a.alg_qual; sc.alg_8d_bytes = a.alg8d; sc.alg_cigar_bytes = a.alg_cigar;
            sc.st = msnv_sample_stats{a.total, a.unmapped, a.zeroq, a.proper, a.dup, a.any_mapped};
            // first pileup read of the sample: the first-line quirk of snpCall (call_vC.cpp:423)
            if (a.first_pile != ~0ull) {
                const int32_t tid = (int32_t)(sum[s].first_key >> 32), pos = (int32_t)(uint32_t)sum[s].first_key;
                int64_t b = pos, e = (int64_t)sum[s].first_end;
                if (ds.has_bed) { b = std::max(b, ds.bed_beg[(size_t)tid]); e = std::min(e, ds.bed_end[(size_t)tid]); }
                if (b < e) { sc.first_tid = tid; sc.first_beg = (int32_t)b; sc.first_end = (int32_t)e; }
            }
            if (a.beyond != ~0ull) {
                sc.warned_beyond_end = true;
                fprintf(stderr, "msnv: warning: read at %s:%d reaches the contig end in qaCompute's index space (undefined behaviour in the reference: coverageHist[-1]); "
                                "the last position of the contig is left out of the coverage histogram\n", ds.names[(size_t)(int32_t)(sum[s].beyond_key >> 32)].c_str(),
                        (int32_t)(uint32_t)sum[s].beyond_key + 1);
            }
        }
        if (in_order) HIP_TRY(hipStreamSynchronize(st));               // (the sorted pairs come down asynchronously)
        {
            std::vector<uint32_t> per(S, 0);
            for (const DevPairRec &r : prec) ++per[r.sample];
            for (size_t s = 0; s < S; ++s) ds.samples[first + s].dev_pairs.reserve(per[s]);
        }
        for (size_t p = 0; p < prec.size(); ++p) {
            const DevPairRec &r = prec[p];
            SampleCols &sc = ds.samples[first + r.sample];
            const uint32_t hi = (p + 1 < prec.size() && prec[p + 1].sample == r.sample) ? prec[p + 1].start : (uint32_t)sum[r.sample + 1].pbase0;
            sc.dev_pairs.push_back(DevPair{r.tid, r.tile, r.start - sum[r.sample].pbase0, hi - sum[r.sample].pbase0, r.maxd, 0u});
        }
        // ... and of every (sample, contig)
        for (const DpRun &r : runs) {
            SampleCols &sc = ds.samples[first + r.sample];
            if (sc.first_any.empty()) { sc.first_any.assign(NC, -1); sc.first_from1.assign(NC, -1); }
            sc.first_any[(size_t)r.tid] = r.first_any; sc.first_from1[(size_t)r.tid] = r.first_from1;
        }
        T.wall_download_s += now_s() - t_dl;
        fin_trace("  pack: host tables");
        return MSNV_OK;
    }
};
}  // namespace

// The driver of a round: the quick route when it may try, the careful route for what it hands back (or for everything), the common tail.
// Which work is queued before which wait is each stage's header comment; a stage that answers TO_CAREFUL has left nothing running.
int devpack_add_round(msnv_dataset &ds, size_t first, const uint8_t *const *streams, const uint64_t *n_bytes, int n, bool on_device, const uint8_t *in_place_base, uint64_t in_place_capacity) {
    (void)in_place_capacity;                                       // (api.cpp / bamfeed.cpp have checked the streams against it)
    if (n <= 0) return MSNV_OK;
    if (n > 2048) return fail(MSNV_EINVAL, "internal: a device-pack round holds at most 2048 samples");
    if (!ds.ctx) return fail(MSNV_ENODEV, "the device pack needs a device context");
    if (int rc = dev_set_device(ds.ctx->device)) return rc;
    fin_trace_reset();
    if (int rc = devpack_sync_pending(ds)) return rc;              // (the round before may still be writing: its work buffers are this round's)
    fin_trace("  pack: enter");
    if (int rc = build_contigs(ds)) return rc;
    fin_trace("  pack: contigs");
    Round R(ds, first, streams, n_bytes, n, on_device, in_place_base);
    if (int rc = R.stage()) return rc;
    int rc = TO_CAREFUL;
    if (R.quick_possible) {
        rc = R.front_quick();
        if (!rc) rc = R.launch_emit();
        if (!rc) rc = R.collect();
    }
    if (rc == TO_CAREFUL) {
        rc = R.front_careful();
        if (!rc) rc = R.edit_qualities();
        if (!rc) rc = R.launch_emit();
        if (!rc) rc = R.collect();
    }
    if (!rc) rc = R.tile_pairs();
    if (!rc) rc = R.publish();
    return rc;
}

// The headers and intervals of the device-packed samples as host staging (SampleCols::hdr / tid / end / depth / cov_*): what the host
// form of finalize_dataset works from.  Taken when the dataset needs one of the re-layouts that still run there (dense pieces, deep
// (sample, tile) runs dealt into groups) or mixes host-packed samples in.
int devpack_download_pieces(msnv_dataset &ds) {
    if (!ds.ctx) return MSNV_OK;
    if (int rc = dev_set_device(ds.ctx->device)) return rc;
    const double t0 = now_s();
    for (SampleCols &sc : ds.samples) {
        if (!sc.dev_index) continue;
        const DevRound &r = ds.dp.rounds[(size_t)sc.dev_round];
        const size_t np = (size_t)sc.n_dev_pieces, ni = (size_t)sc.n_dev_iv;
        sc.hdr.resize(np); sc.tid.resize(np); sc.end.resize(np); sc.depth.resize(np);
        sc.cov_tid.resize(ni); sc.cov_beg.resize(ni); sc.cov_end.resize(ni);
        if (np) {
            HIP_TRY(hipMemcpy(sc.hdr.data(), r.hdr + sc.dev_piece0, np * sizeof(ReadHdr), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(sc.tid.data(), r.tid + sc.dev_piece0, np * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(sc.end.data(), r.end + sc.dev_piece0, np * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(sc.depth.data(), r.depth + sc.dev_piece0, np * 2, hipMemcpyDeviceToHost));
        }
        if (ni) {
            HIP_TRY(hipMemcpy(sc.cov_tid.data(), r.cov_tid + sc.dev_iv0, ni * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(sc.cov_beg.data(), r.cov_beg + sc.dev_iv0, ni * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(sc.cov_end.data(), r.cov_end + sc.dev_iv0, ni * 4, hipMemcpyDeviceToHost));
        }
        sc.dev_index = false; sc.dev_pairs.clear(); sc.dev_pairs.shrink_to_fit();
    }
    for (DevRound &r : ds.dp.rounds) if (r.buf) { dev_free(r.buf); r.buf = nullptr; }
    ds.dp.wall_download_s += now_s() - t0;
    return MSNV_OK;
}

// The two kernels of the round that finalize's deep-run split borrows (devwork.h)
int devpack_gather_pieces(hipStream_t st, const uint32_t *src, const DevRound &R, ReadHdr *hdr2, int32_t *tid2, int32_t *end2, uint16_t *depth2) {
    hipLaunchKernelGGL(msnv_gather_pieces, grid_for(R.n_pieces, 256), dim3(256), 0, st, src, (uint32_t)R.n_pieces, R.hdr, R.tid, R.end, R.depth, hdr2, tid2, end2, depth2);
    HIP_TRY(hipGetLastError());
    return MSNV_OK;
}
int devpack_emit_tail(msnv_dataset &ds, uint8_t *seq, uint8_t *qual, unsigned long long piece_bytes) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    const msnv_params &MP = ds.params;
    DpParams P{}; P.c_eff = std::min(std::max(MP.min_baseq, -127), 127); P.all_low = MP.min_baseq > 127;
    const DpSampleDst dst{seq, qual, 0ull, 0u, 0u};
    DevBuf d_dst, d_pb;
    if (int rc = d_dst.alloc(sizeof(DpSampleDst))) return rc;
    if (int rc = d_pb.alloc(8)) return rc;
    HIP_TRY(hipMemcpyAsync(d_dst.p, &dst, sizeof dst, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pb.p, &piece_bytes, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(msnv_emit_tail, dim3(1), dim3(64), 0, st, d_dst.as<DpSampleDst>(), d_pb.as<unsigned long long>(), 1u, P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MSNV_OK;
}

int devpack_sample_to_host(SampleCols &sc) {
    if (!sc.on_device) return MSNV_OK;
    const uint64_t nb = sc.d_seq_bytes;
    sc.seq.resize(nb);
    std::vector<uint8_t> bits((2 * nb + 7) / 8);
    if (nb) HIP_TRY(hipMemcpy(sc.seq.data(), sc.d_seq, nb, hipMemcpyDeviceToHost));
    if (!bits.empty()) HIP_TRY(hipMemcpy(bits.data(), sc.d_qual, bits.size(), hipMemcpyDeviceToHost));
    // flags back to staging bytes: 0x80 is below every cutoff, 127 below none that flags a real quality (finalize.cpp: pack_lowq)
    sc.qual.resize(2 * nb);
    for (uint64_t i = 0; i < 2 * nb; ++i) sc.qual[i] = (bits[i >> 3] >> (i & 7)) & 1u ? 0x80 : 127;
    sc.on_device = false; sc.d_seq = nullptr; sc.d_qual = nullptr; sc.d_seq_bytes = 0;
    return MSNV_OK;
}

// The runtime loads a translation unit's code object when its first kernel is launched (~10 ms): msnv_ctx_create does that here, on the
// thread that brings the context up, instead of inside the first timed stage.
__global__ void msnv_warm_devpack() {}
void warm_devpack(void *stream) { hipLaunchKernelGGL(msnv_warm_devpack, dim3(1), dim3(1), 0, (hipStream_t)stream); (void)hipGetLastError(); }

}  // namespace msnv
