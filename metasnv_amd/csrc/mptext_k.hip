// metasnv_amd/csrc/mptext_k.hip -- the text of `samtools mpileup -f REF [-l BED] -B -b LIST` (bam_plcmd.c: the mpileup text loop and
// pileup_seq; sam.c: resolve_cigar2 [EXT]) formatted on the device, for a group of position tiles at a time.
//
// A tile is MPT_T positions of one contig.  One wavefront handles one (tile, sample): lane i owns position t0 + i and walks the pair's read
// list -- file order, taken through LDS MPT_B descriptors at a time -- sequentially, so the order of the elements inside a cell is the file
// order of the reads whatever the hardware schedules; no atomic decides a placement.  The walk exists ONCE (mpt_traverse<WRITE>): the
// measure pass counts the bytes the write pass stores.
//
//   mpt_cells<false>   per cell: kept elements (cnt), length of the bases string, "a pushed read covers the position"
//   mpt_cell_offsets   per line: the cells' offsets behind the header, the line's length (0: no read there, or outside the BED)
//   mpt_scan_lines     exclusive scan of the line lengths, 64-bit
//   mpt_cells<true>    the bytes, at the offsets; every column's writer checks that it ended where the next column or cell starts
//   mpt_empty_lines    MPT_ALL: the lines of the tiles no read list reaches, a lane per line, all S cells of it
//
// A lane spends work on reads of its pair that do not cover its position (at most MPT_T - 1 positions to either side): fine for short reads.
//
// The options of msnv_mpileup_text_opts are the template argument OPT (MPT_ALL | MPT_MQ | MPT_BP, mptext.h): OPT = 0 is the text of
// `samtools mpileup` without -a / -s / -O and compiles to the kernels as they were before the options existed.
#include <type_traits>

#include <hip/hip_runtime.h>

#include "mptext.h"
#include "hiptry.h"

namespace msnv {

namespace {

__device__ __forceinline__ uint32_t ld_u32_dev(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
// the decimal digits of v at p; returns the byte behind them
__device__ __forceinline__ char *put_dec(char *p, uint32_t v) {
    const uint32_t n = dec_digits(v);
    for (uint32_t i = n; i-- > 0;) { p[i] = (char)('0' + v % 10u); v /= 10u; }
    return p + n;
}
// htslib's seq_nt16_table for the characters a FASTA holds (unknown: 15)
__device__ __forceinline__ uint32_t nt16_of(uint32_t c) {
    switch (c) {
        case '=': return 0;
        case '0': return 1; case '1': return 2; case '2': return 4; case '3': return 8;
        default: break;
    }
    switch (c | 0x20u) {
        case 'a': return 1;  case 'c': return 2;  case 'g': return 4;  case 't': return 8;
        case 'm': return 3;  case 'r': return 5;  case 's': return 6;  case 'v': return 7;
        case 'w': return 9;  case 'y': return 10; case 'h': return 11; case 'k': return 12;
        case 'd': return 13; case 'b': return 14;
        default: return 15;
    }
}
__device__ __forceinline__ char to_strand(uint32_t c, bool rev) {      // tolower / toupper of the C locale
    if (rev) return (char)(c >= 'A' && c <= 'Z' ? c + 32u : c);
    return (char)(c >= 'a' && c <= 'z' ? c - 32u : c);
}
__device__ __forceinline__ bool consumes_ref_dev(uint32_t op) { return op == C_M || op == C_D || op == C_N || op == C_EQ || op == C_X; }
__device__ __forceinline__ uint32_t seq_code(const uint8_t *seq, int32_t i) { return (seq[i >> 1] >> ((~i & 1) << 2)) & 0xfu; }

__device__ __forceinline__ uint32_t header_len(const MptContig &c, int32_t pos) { return c.name_len + 1u + dec_digits((uint32_t)pos + 1u) + 2u; }

// The element of read d at position p (sam.c resolve_cigar2, restated from the CIGAR's start): false when p lies behind the last
// reference-consuming operation (cannot happen inside [pos, end)).
struct Elem { int32_t qpos, indel; bool is_del, is_refskip; };
__device__ __forceinline__ bool resolve_elem(const MptRead &d, const uint8_t *cig, int32_t p, Elem &e) {
    long long x = d.pos; int32_t y = 0; uint32_t k = 0;
    uint32_t op = 0; long long l = 0;
    for (;;) {
        if (k >= d.n_cigar) return false;
        const uint32_t c = ld_u32_dev(cig + 4 * (size_t)k); op = c & 15u; l = c >> 4;
        const bool refc = consumes_ref_dev(op);
        if (refc && p < x + l) break;
        if (refc) x += l;
        if (op == C_M || op == C_I || op == C_S || op == C_EQ || op == C_X) y += (int32_t)l;
        ++k;
    }
    e.indel = 0; e.is_del = false; e.is_refskip = false;
    if (op == C_M || op == C_EQ || op == C_X) {
        e.qpos = y + (int32_t)(p - x);
        if (x + l - 1 == p && k + 1 < d.n_cigar) {
            uint32_t c2 = ld_u32_dev(cig + 4 * (size_t)(k + 1)), op2 = c2 & 15u;
            if (op2 == C_D) e.indel = -(int32_t)(c2 >> 4);
            else if (op2 == C_I) e.indel = (int32_t)(c2 >> 4);
            else if (op2 == C_P && k + 2 < d.n_cigar) {
                int32_t l3 = 0;
                for (uint32_t k2 = k + 2; k2 < d.n_cigar; ++k2) {
                    c2 = ld_u32_dev(cig + 4 * (size_t)k2); op2 = c2 & 15u;
                    if (op2 == C_I) l3 += (int32_t)(c2 >> 4);
                    else if (op2 == C_D || op2 == C_M || op2 == C_N || op2 == C_EQ || op2 == C_X) break;
                }
                if (l3 > 0) e.indel = l3;
            }
        }
    } else { e.is_del = true; e.qpos = y; e.is_refskip = op == C_N; }
    return true;
}

// One lane's walk over the read list of its (tile, sample).  Every lane of the wavefront takes part in the LDS hand-over; a lane whose
// position has no line (`mine` false) handles no read.  WRITE: the element's characters go to bases / quals, which advance; otherwise only
// cnt / blen / covered are counted -- by the same expressions.  MPT_MQ: one character per kept element goes to mqc; MPT_BP: bplen counts
// ",<qpos + 1>" per kept element (the caller takes the first comma off), bpc receives the numbers.
template <bool WRITE, uint32_t OPT>
__device__ __forceinline__ void mpt_traverse(const MptJob &J, const MptRange rg, const uint8_t *rec, const MptRead *reads, const MptContig &ct, int32_t p, bool mine,
                                             MptRead *sh, uint32_t &cnt, uint32_t &blen, uint32_t &bplen, bool &covered, char *&bases, char *&quals, char *&mqc, char *&bpc) {
    const int lane = threadIdx.x;
    const char *ref = ct.ref_len >= 0 ? J.ref + ct.ref_off : nullptr;
    for (uint32_t b0 = rg.lo; b0 < rg.hi; b0 += MPT_B) {
        const uint32_t nb = min((uint32_t)MPT_B, rg.hi - b0);
        __syncthreads();
        for (uint32_t j = lane; j < nb; j += MPT_T) {
            const uint4 *src = reinterpret_cast<const uint4 *>(reads + b0 + j);
            uint4 *dst = reinterpret_cast<uint4 *>(sh + j);
            dst[0] = src[0]; dst[1] = src[1];
        }
        __syncthreads();
        if (!mine) continue;
        for (uint32_t j = 0; j < nb; ++j) {
            const MptRead d = sh[j];
            if (!(d.pos <= p && p < d.end)) continue;
            covered = true;
            const uint8_t *cig = rec + d.cig_off;
            Elem e;
            if (!resolve_elem(d, cig, p, e)) continue;
            const uint8_t *seq = cig + d.seq_rel, *qual = seq + ((size_t)d.l_seq + 1) / 2;
            const uint32_t q = e.qpos < d.l_seq ? qual[e.qpos] : 0u;
            if ((int32_t)q < J.min_baseq) continue;
            const bool head = p == d.pos, tail = p == d.end - 1, rev = (d.flags >> 8) & 1u;
            const uint32_t n_indel = (uint32_t)(e.indel < 0 ? -e.indel : e.indel);
            ++cnt;
            blen += (head ? 2u : 0u) + 1u + (n_indel ? 1u + dec_digits(n_indel) + n_indel : 0u) + (tail ? 1u : 0u);
            if (OPT & MPT_BP) bplen += 1u + dec_digits((uint32_t)e.qpos + 1u);
            if (WRITE) {
                char *o = bases;
                if (head) { const uint32_t mq = d.flags & 0xffu; *o++ = '^'; *o++ = (char)(mq > 93u ? 126u : mq + 33u); }
                if (!e.is_del) {
                    const uint32_t code = e.qpos < d.l_seq ? seq_code(seq, e.qpos) : 15u;
                    bool match = code == 0u;
                    if (!match && ref) match = code == nt16_of(p < ct.ref_len ? (uint8_t)ref[p] : (uint32_t)'N');
                    *o++ = match ? (rev ? ',' : '.') : to_strand((uint8_t)"=ACMGRSVTWYHKDBN"[code], rev);
                } else *o++ = e.is_refskip ? (rev ? '<' : '>') : '*';
                if (e.indel > 0) {
                    *o++ = '+'; o = put_dec(o, n_indel);
                    for (int32_t j2 = 1; j2 <= e.indel; ++j2) {
                        const long long qi = (long long)e.qpos + j2;
                        *o++ = to_strand(qi < d.l_seq ? (uint8_t)"=ACMGRSVTWYHKDBN"[seq_code(seq, (int32_t)qi)] : (uint32_t)'N', rev);
                    }
                } else if (e.indel < 0) {
                    *o++ = '-'; o = put_dec(o, n_indel);
                    for (uint32_t j2 = 1; j2 <= n_indel; ++j2) {
                        const long long rp = (long long)p + j2;
                        *o++ = to_strand(ref && rp < ct.ref_len ? (uint8_t)ref[rp] : (uint32_t)'N', rev);
                    }
                }
                if (tail) *o++ = '$';
                bases = o;
                *quals++ = (char)min(q + 33u, 126u);
                if (OPT & MPT_MQ) *mqc++ = (char)min((d.flags & 0xffu) + 33u, 126u);
                if (OPT & MPT_BP) { if (cnt > 1u) *bpc++ = ','; bpc = put_dec(bpc, (uint32_t)e.qpos + 1u); }
            }
        }
    }
}

// grid: n_items * S workgroups of MPT_T lanes; workgroup b = (work item item_lo + b / S of the group, sample b % S).  A work item is a
// tile; with MPT_ALL it is an entry of J.work, the tiles that hold reads (the empty ones are mpt_empty_lines').  WRITE: the lines go to
// text, whose first byte is byte base_off of the group's text.
template <bool WRITE, uint32_t OPT>
__global__ __launch_bounds__(MPT_T) void mpt_cells(const MptJob J, uint32_t item_lo, unsigned long long base_off, char *text) {
    __shared__ __align__(16) MptRead sh[MPT_B];
    const uint32_t item = item_lo + blockIdx.x / J.S, s = blockIdx.x % J.S;
    const uint32_t tile = (OPT & MPT_ALL) ? J.work[item] : item;
    const MptTile tl = J.tiles[tile];
    const MptRange rg = J.ranges[(size_t)item * J.S + s];
    const MptContig ct = J.contigs[tl.contig];
    const int32_t p = tl.t0 + (int32_t)threadIdx.x;
    const uint32_t line = tile * MPT_T + threadIdx.x;
    const size_t cell = (size_t)s * J.lines_cap + line;
    bool mine = p >= tl.vbeg && p < tl.vend;
    uint32_t cnt = 0, blen = 0, bplen = 0; bool covered = false;
    char *bases = nullptr, *quals = nullptr, *bases_end = nullptr, *next_cell = nullptr;
    char *mqc = nullptr, *bpc = nullptr, *quals_end = nullptr, *mq_end = nullptr;      // MPT_MQ / MPT_BP: the columns behind the qualities
    if (WRITE) {
        const unsigned long long off = J.line_off[line], off_next = J.line_off[line + 1];
        mine = mine && off_next > off;
        if (mine) {
            char *lp = text + (off - base_off);
            const uint32_t hl = header_len(ct, p), want_cnt = J.cnt[cell], want_blen = J.blen[cell];
            if (s == 0) {
                const char *nm = J.names + ct.name_off;
                for (uint32_t i = 0; i < ct.name_len; ++i) lp[i] = nm[i];
                char *o = lp + ct.name_len;
                *o++ = '\t'; o = put_dec(o, (uint32_t)p + 1u); *o++ = '\t';
                *o++ = ct.ref_len >= 0 && p < ct.ref_len ? J.ref[ct.ref_off + p] : 'N';
            }
            char *o = lp + hl + J.rel[cell];
            *o++ = '\t'; o = put_dec(o, want_cnt); *o++ = '\t';
            bases = o;
            bases_end = bases + max(want_blen, 1u);
            *bases_end = '\t';
            quals = bases_end + 1;
            next_cell = s + 1 < J.S ? lp + hl + J.rel[cell + J.lines_cap] : text + (off_next - base_off) - 1;
            if (s + 1 == J.S) *next_cell = '\n';
            if (OPT & (MPT_MQ | MPT_BP)) {                                            // each column: a tab, then max(its length, 1) bytes
                char *e = quals + max(want_cnt, 1u);
                quals_end = e;
                if (OPT & MPT_MQ) { *e = '\t'; mqc = e + 1; e = mqc + max(want_cnt, 1u); mq_end = e; }
                if (OPT & MPT_BP) { *e = '\t'; bpc = e + 1; }                         // (ends at next_cell)
            }
            if (want_cnt == 0) {                                                      // no read there, or every element below -Q
                *bases++ = '*'; *quals++ = '*'; mine = false;
                if (OPT & MPT_MQ) *mqc++ = '*';
                if (OPT & MPT_BP) *bpc++ = '*';
            }
        }
    }
    mpt_traverse<WRITE, OPT>(J, rg, J.rec[s], J.reads[s], ct, p, mine, sh, cnt, blen, bplen, covered, bases, quals, mqc, bpc);
    if (WRITE) {
        if (bases_end) {                                                              // (every writer stores the same value)
            bool bad = bases != bases_end;
            if (!(OPT & (MPT_MQ | MPT_BP))) bad |= quals != next_cell;
            else {
                bad |= quals != quals_end;
                if (OPT & MPT_MQ) bad |= mqc != ((OPT & MPT_BP) ? mq_end : next_cell);
                if (OPT & MPT_BP) bad |= bpc != next_cell;
            }
            if (bad) *J.flag = 1u;
        }
    } else {
        J.cnt[cell] = cnt; J.blen[cell] = blen;
        if (OPT & MPT_BP) J.bplen[cell] = bplen ? bplen - 1u : 0u;                     // (no comma in front of the first number)
        if (covered) J.active[line] = 1u;                                              // (likewise)
    }
}

// bytes of a zero-depth cell: "\t0\t*\t*" and "\t*" per extra column
template <uint32_t OPT> __device__ __forceinline__ constexpr uint32_t empty_cell_len() { return 6u + ((OPT & MPT_MQ) ? 2u : 0u) + ((OPT & MPT_BP) ? 2u : 0u); }

// one lane per line of the group.  MPT_ALL: a line is active under a read or not -- every position of [vbeg, vend) up to the contig's
// length in a tile that holds reads, every position of [vbeg, vend) (the host has cut it) in an empty tile, whose cells have no tables.
template <uint32_t OPT>
__global__ __launch_bounds__(256) void mpt_cell_offsets(const MptJob J, uint32_t n_lines) {
    const uint32_t line = blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= n_lines) return;
    uint32_t len = 0;
    bool active = J.active[line] != 0u;
    if (OPT & MPT_ALL) {
        const MptTile t = J.tiles[line / MPT_T];
        const int32_t p = t.t0 + (int32_t)(line % MPT_T);
        active = t.contig < 0 ? p >= t.vbeg && p < t.vend : active || (p >= t.vbeg && p < t.vend && p < J.contigs[t.contig].len);
    }
    if (active) {
        const MptTile tl = J.tiles[line / MPT_T];
        const bool empty = (OPT & MPT_ALL) && tl.contig < 0;
        uint32_t acc = 0; unsigned long long kept = 0;
        if (empty) acc = J.S * empty_cell_len<OPT>();
        else for (uint32_t s = 0; s < J.S; ++s) {
            const size_t cell = (size_t)s * J.lines_cap + line;
            const uint32_t cnt = J.cnt[cell], blen = J.blen[cell];
            J.rel[cell] = acc;
            acc += 1u + dec_digits(cnt) + 1u + max(blen, 1u) + 1u + max(cnt, 1u);
            if (OPT & MPT_MQ) acc += 1u + max(cnt, 1u);
            if (OPT & MPT_BP) acc += 1u + max(J.bplen[cell], 1u);
            kept += cnt;
        }
        len = header_len(J.contigs[empty ? ~tl.contig : tl.contig], tl.t0 + (int32_t)(line % MPT_T)) + acc + 1u;
        atomicAdd(&J.totals[0], 1ull); atomicAdd(&J.totals[1], kept);               // statistics only
    }
    J.line_len[line] = len;
}

// one workgroup: every lane sums a run of consecutive lines, lane 0 scans the 1024 sums, every lane writes its run's offsets
constexpr int MPT_SCAN_NT = 1024;
__global__ __launch_bounds__(MPT_SCAN_NT) void mpt_scan_lines(const MptJob J, uint32_t n_lines) {
    __shared__ unsigned long long part[MPT_SCAN_NT];
    const uint32_t per = (n_lines + MPT_SCAN_NT - 1) / MPT_SCAN_NT;
    const uint32_t lo = min(n_lines, threadIdx.x * per), hi = min(n_lines, lo + per);
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += J.line_len[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (int i = 0; i < MPT_SCAN_NT; ++i) { const unsigned long long v = part[i]; part[i] = acc; acc += v; }
        J.line_off[n_lines] = acc; J.tile_off[n_lines / MPT_T] = acc;
    }
    __syncthreads();
    unsigned long long off = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        J.line_off[i] = off;
        if (i % MPT_T == 0) J.tile_off[i / MPT_T] = off;
        off += J.line_len[i];
    }
}

// MPT_ALL: one lane per line of tiles [tile_lo, tile_hi); a lane whose tile is empty writes its whole line -- the head and S zero-depth
// cells -- and checks that it ended where the next line starts.
template <uint32_t OPT>
__global__ __launch_bounds__(256) void mpt_empty_lines(const MptJob J, uint32_t tile_lo, uint32_t tile_hi, unsigned long long base_off, char *text) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (tile_hi - tile_lo) * MPT_T) return;
    const uint32_t line = tile_lo * MPT_T + i;
    const MptTile tl = J.tiles[line / MPT_T];
    if (tl.contig >= 0) return;
    const unsigned long long off = J.line_off[line], off_next = J.line_off[line + 1];
    if (off_next == off) return;
    const MptContig ct = J.contigs[~tl.contig];
    const int32_t p = tl.t0 + (int32_t)(line % MPT_T);
    char *o = text + (off - base_off);
    const char *nm = J.names + ct.name_off;
    for (uint32_t k = 0; k < ct.name_len; ++k) *o++ = nm[k];
    *o++ = '\t'; o = put_dec(o, (uint32_t)p + 1u); *o++ = '\t';
    *o++ = ct.ref_len >= 0 && p < ct.ref_len ? J.ref[ct.ref_off + p] : 'N';
    for (uint32_t s = 0; s < J.S; ++s) {
        *o++ = '\t'; *o++ = '0'; *o++ = '\t'; *o++ = '*'; *o++ = '\t'; *o++ = '*';
        if (OPT & MPT_MQ) { *o++ = '\t'; *o++ = '*'; }
        if (OPT & MPT_BP) { *o++ = '\t'; *o++ = '*'; }
    }
    *o++ = '\n';
    if (o != text + (off_next - base_off)) *J.flag = 1u;
}

__global__ void msnv_warm_mptext() {}

// f(std::integral_constant<uint32_t, opt>): the instantiation of a kernel for the call's options
template <typename F> void with_opt(uint32_t opt, F &&f) {
    switch (opt & 7u) {
        case 0: f(std::integral_constant<uint32_t, 0>{}); break;
        case 1: f(std::integral_constant<uint32_t, 1>{}); break;
        case 2: f(std::integral_constant<uint32_t, 2>{}); break;
        case 3: f(std::integral_constant<uint32_t, 3>{}); break;
        case 4: f(std::integral_constant<uint32_t, 4>{}); break;
        case 5: f(std::integral_constant<uint32_t, 5>{}); break;
        case 6: f(std::integral_constant<uint32_t, 6>{}); break;
        default: f(std::integral_constant<uint32_t, 7>{}); break;
    }
}

}  // namespace

int mpt_measure(const MptJob &j, uint32_t n_tiles, uint32_t n_work, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t n_lines = n_tiles * MPT_T;
    if (n_tiles == 0 || n_lines > j.lines_cap || n_work > n_tiles) return fail(MSNV_EINVAL, "mpt_measure: %u tiles do not fit the group's tables", n_tiles);
    HIP_TRY(hipMemsetAsync(j.active, 0, (size_t)n_lines * sizeof(uint32_t), stream));
    with_opt(j.opt & ~MPT_MQ, [&](auto o) {                      // (the MAPQ column is as long as the qualities: nothing to measure)
        if (n_work) hipLaunchKernelGGL((mpt_cells<false, decltype(o)::value>), dim3(n_work * j.S), dim3(MPT_T), 0, stream, j, 0u, 0ull, (char *)nullptr);
    });
    with_opt(j.opt, [&](auto o) { hipLaunchKernelGGL((mpt_cell_offsets<decltype(o)::value>), dim3((n_lines + 255) / 256), dim3(256), 0, stream, j, n_lines); });
    hipLaunchKernelGGL(mpt_scan_lines, dim3(1), dim3(MPT_SCAN_NT), 0, stream, j, n_lines);
    HIP_TRY(hipGetLastError());
    return MSNV_OK;
}

int mpt_write(const MptJob &j, uint32_t tile_lo, uint32_t tile_hi, uint32_t work_lo, uint32_t work_hi, unsigned long long base_off, char *text, void *stream) {
    if (tile_hi <= tile_lo) return MSNV_OK;
    with_opt(j.opt, [&](auto o) {
        constexpr uint32_t O = decltype(o)::value;
        if (work_hi > work_lo) hipLaunchKernelGGL((mpt_cells<true, O>), dim3((work_hi - work_lo) * j.S), dim3(MPT_T), 0, (hipStream_t)stream, j, work_lo, base_off, text);
        if constexpr ((O & MPT_ALL) != 0u) hipLaunchKernelGGL((mpt_empty_lines<O>), dim3(((tile_hi - tile_lo) * MPT_T + 255) / 256), dim3(256), 0, (hipStream_t)stream, j, tile_lo, tile_hi, base_off, text);
    });
    HIP_TRY(hipGetLastError());
    return MSNV_OK;
}

int mpt_pinned_alloc(void **p, uint64_t bytes) {
    *p = nullptr;
    const hipError_t e = hipHostMalloc(p, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) { *p = nullptr; return fail(MSNV_ENOMEM, "pinned host memory of %llu bytes for the mpileup text: %s", (unsigned long long)bytes, hipGetErrorString(e)); }
    return MSNV_OK;
}
void mpt_pinned_free(void *p) { if (p) (void)hipHostFree(p); }
int mpt_event_create(void **ev) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); *ev = e; return MSNV_OK; }
void mpt_event_destroy(void *ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
int mpt_event_record(void *ev, void *stream) { HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return MSNV_OK; }
int mpt_event_wait(void *ev) { HIP_TRY(hipEventSynchronize((hipEvent_t)ev)); return MSNV_OK; }
int mpt_stream_wait_event(void *stream, void *ev) { HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0)); return MSNV_OK; }
int mpt_event_ms(void *ev0, void *ev1, double *ms) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, (hipEvent_t)ev0, (hipEvent_t)ev1)); *ms = f; return MSNV_OK; }
int mpt_copy_to_host_async(void *dst_pinned, const void *src_device, uint64_t bytes, void *stream) {
    if (bytes) HIP_TRY(hipMemcpyAsync(dst_pinned, src_device, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return MSNV_OK;
}
void warm_mptext(void *stream) { hipLaunchKernelGGL(msnv_warm_mptext, dim3(1), dim3(1), 0, (hipStream_t)stream); (void)hipGetLastError(); }

}  // namespace msnv
