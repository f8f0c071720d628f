// metasnv_amd/csrc/mptext.cpp -- msnv_mpileup_text[_ex] / msnv_mpileup_text_records[_ex] (include/msnv.h): the text `samtools mpileup -f REF
// [-l BED] -B -b LIST` pipes into snpCall (metaSNV.py:160-165), formatted on the device (mptext_k.hip).  This file is the host side:
//
//   rounds   the samples come in rounds of MSNV_MPTEXT_ROUND.  Per round the sequential read-level steps run on host threads -- pack.cpp's
//            host_prepass on a context-less dataset: read filters, depth cap, the overlapping-mates quality edit; token_limit is 0, mpileup
//            cuts nothing -- and the record streams (edited qualities), and per sample the table of its pushed reads in file order, go up.
//   tiles    MPT_T positions of one contig; per (tile, sample) the read list: from the first read with end > t0 to the first with
//            pos >= t0 + MPT_T.  Tiles no list reaches are never made -- unless every position is asked for (msnv_mpileup_text_opts
//            all_positions): then they are EMPTY tiles (MptTile contig < 0), which carry no read lists, get no workgroups and are
//            written a lane per line, but are tiles of their group like any other: the same scan, the same offsets, the same batches.
//            Tiles go to the device in groups that bound the per-cell tables.
//   batches  a group is measured and scanned at once; its text is written in batches of whole tiles of at most MSNV_MPTEXT_BATCH bytes
//            (a tile that is longer is a batch of its own), through two device buffers and two pinned buffers: the copy and the file
//            write of batch k run under the kernels of batch k + 1.  Neither the text nor a genome-wide cell table is ever resident.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "bamfeed.h"
#include "devpack.h"
#include "mptext.h"

using namespace msnv;

namespace {

struct Sink {                           // a file, or memory the caller releases with msnv_free
    FILE *f = nullptr; bool close_f = false;
    char *mem = nullptr; uint64_t n = 0, cap = 0; bool to_mem = false;
    int put(const char *p, uint64_t bytes) {
        if (!bytes) return MSNV_OK;
        if (to_mem) {
            if (n + bytes > cap) {
                const uint64_t want = std::max<uint64_t>(n + bytes, cap + cap / 2 + 4096);
                char *q = (char *)realloc(mem, want);
                if (!q) return fail(MSNV_ENOMEM, "mpileup text: %llu bytes of host memory", (unsigned long long)want);
                mem = q; cap = want;
            }
            memcpy(mem + n, p, bytes);
        } else if (fwrite(p, 1, bytes, f) != bytes) return fail(MSNV_EIO, "mpileup text: write failed");
        n += bytes;
        return MSNV_OK;
    }
    ~Sink() { if (f && close_f) fclose(f); free(mem); }
};

// host copy of what the tiling needs of a sample's pushed reads
struct SampleTab {
    std::vector<MptRead> reads;             // file order (cleared once uploaded)
    std::vector<int32_t> pos, pmax;         // per read: start; furthest end of its contig's reads up to and including it
    std::vector<int32_t> run_tid; std::vector<uint32_t> run_lo;      // its reads contig by contig (ascending); run_lo has one entry more
};

int build_table(const msnv_dataset &ds, const uint8_t *rec, uint64_t n_bytes, std::vector<uint8_t> &patched, SampleTab &t) {
    std::vector<uint32_t> ovr; bool cut_marks = false;
    if (int rc = host_prepass(ds, rec, n_bytes, ovr, patched, cut_marks)) return rc;
    uint64_t off = 0; size_t idx = 0;
    while (off < n_bytes) {
        RecView r;
        if (!rec_parse(rec + off, n_bytes - off, r)) return fail(MSNV_EFORMAT, "malformed BAM record at byte %llu", (unsigned long long)off);
        if (idx < ovr.size() && (ovr[idx] & 2u)) {                     // pile_ok: passes the read filters, not depth-capped
            int64_t rlen = 0;
            for (int k = 0; k < r.n_cigar; ++k) { const uint32_t c = ld_u32(r.cigar + 4 * k), op = c & 15u; if (op == C_M || op == C_D || op == C_N || op == C_EQ || op == C_X) rlen += c >> 4; }
            const int64_t end = (int64_t)r.pos + (rlen ? rlen : 1);
            if (end > INT32_MAX) return fail(MSNV_EDOMAIN, "a read ends at position %lld, beyond what a BAM position holds", (long long)end);
            MptRead d;
            d.cig_off = (uint64_t)(r.cigar - rec); d.pos = r.pos; d.end = (int32_t)end; d.n_cigar = (uint32_t)r.n_cigar; d.l_seq = r.l_seq;
            d.seq_rel = (int32_t)(r.seq - r.cigar); d.flags = (uint32_t)r.mapq | ((r.flag & BAM_FREVERSE) ? 256u : 0u);
            if (t.run_tid.empty() || t.run_tid.back() != r.tid) { t.run_tid.push_back(r.tid); t.run_lo.push_back((uint32_t)t.reads.size()); }
            const bool first = t.run_lo.back() == t.reads.size();
            t.pmax.push_back(first ? d.end : std::max(t.pmax.back(), d.end));
            t.pos.push_back(d.pos);
            t.reads.push_back(d);
        }
        off += r.size; ++idx;
    }
    if (t.reads.size() >= 0xffffffffull) return fail(MSNV_EDOMAIN, "a sample holds more than 2^32 - 1 pileup reads");
    t.run_lo.push_back((uint32_t)t.reads.size());
    return MSNV_OK;
}

struct Run {
    msnv_ctx *ctx; msnv_dataset *ds; Sink &sink;
    std::vector<SampleTab> tabs;
    std::vector<void *> dev;                       // everything allocated on the device
    std::vector<const uint8_t *> d_rec; std::vector<const MptRead *> d_reads;
    void *pin_text[2] = {nullptr, nullptr}, *pin_small = nullptr, *ev[8] = {};
    uint64_t rounds = 0, batches = 0; double ms_measure = 0, ms_write = 0;
    unsigned long long totals[2] = {0, 0};
    uint32_t opt = 0; int32_t all_level = 0;       // MPT_ALL | MPT_MQ | MPT_BP; 1: -a, 2: -aa

    Run(msnv_ctx *c, msnv_dataset *d, Sink &s, uint32_t o, int32_t lvl) : ctx(c), ds(d), sink(s), opt(o), all_level(lvl) {}
    ~Run() {
        if (ctx) { (void)dev_stream_wait(ctx->stream); if (ctx->stream2) (void)dev_stream_wait(ctx->stream2); }
        for (void *p : dev) dev_free(p);
        mpt_pinned_free(pin_text[0]); mpt_pinned_free(pin_text[1]); mpt_pinned_free(pin_small);
        for (void *e : ev) mpt_event_destroy(e);
    }
    int alloc(void **p, uint64_t bytes) { if (int rc = dev_alloc(p, bytes, nullptr)) return rc; dev.push_back(*p); return MSNV_OK; }
    template <typename T> int up(T **p, const std::vector<T> &v) {
        void *q = nullptr;
        if (int rc = alloc(&q, v.size() * sizeof(T))) return rc;
        *p = (T *)q;
        return dev_upload(q, v.data(), v.size() * sizeof(T));
    }

    // n record streams become samples tabs.size() ..: pre-pass and read tables on host threads, then one device buffer for the round
    int add_round(const uint8_t *const *rec, const uint64_t *n_bytes, int n, int threads) {
        const size_t first = tabs.size();
        tabs.resize(first + (size_t)n);
        std::vector<std::vector<uint8_t>> patched((size_t)n);
        if (int rc = for_each_index(0, (size_t)n, pool_threads(threads, n), 1,
                                    [&](size_t i) { return build_table(*ds, rec[i], n_bytes[i], patched[i], tabs[first + i]); },
                                    [&](size_t i) { return "mpileup text: sample " + std::to_string(first + i); })) return rc;
        uint64_t total = 0;
        std::vector<uint64_t> rec_at((size_t)n), tab_at((size_t)n);
        for (int i = 0; i < n; ++i) { rec_at[(size_t)i] = total; total += (n_bytes[i] + 31) / 32 * 32 + 32; }
        for (int i = 0; i < n; ++i) { tab_at[(size_t)i] = total; total += tabs[first + (size_t)i].reads.size() * sizeof(MptRead) + 32; }
        void *buf = nullptr;
        if (int rc = alloc(&buf, total)) return rc;
        for (int i = 0; i < n; ++i) {
            SampleTab &t = tabs[first + (size_t)i];
            uint8_t *dr = (uint8_t *)buf + rec_at[(size_t)i], *dt = (uint8_t *)buf + tab_at[(size_t)i];
            if (int rc = dev_upload(dr, patched[(size_t)i].empty() ? rec[i] : patched[(size_t)i].data(), n_bytes[i])) return rc;
            if (int rc = dev_upload(dt, t.reads.data(), t.reads.size() * sizeof(MptRead))) return rc;
            d_rec.push_back(dr); d_reads.push_back((const MptRead *)dt);
            std::vector<MptRead>().swap(t.reads);
        }
        ++rounds;
        return MSNV_OK;
    }

    int format();
};

// Tiles in (contig, position) order, made on demand.  all: the positions [fb, fe) of a contig in play -- its @SQ length cut to its BED
// region -- have lines whether a read covers them or not, so the stretches of them no read list reaches become empty tiles.
struct Tiler {
    const msnv_dataset &ds; const std::vector<SampleTab> &tabs; const std::vector<int32_t> &play;      // play: the contigs that print lines, ascending
    const bool all;
    size_t ci = 0; bool open = false; int64_t t0 = 0;
    std::vector<size_t> run; std::vector<uint32_t> lo, hi, end;      // per sample: cursor into its runs; list cursors and end of the contig's run
    Tiler(const msnv_dataset &d, const std::vector<SampleTab> &t, const std::vector<int32_t> &p, bool a) : ds(d), tabs(t), play(p), all(a), run(t.size(), 0), lo(t.size()), hi(t.size()), end(t.size()) {}
    // the next tile; a tile that holds reads appends its index to work and its S ranges to ranges; false: no tile is left
    bool next(std::vector<MptTile> &tiles, std::vector<MptRange> &ranges, std::vector<uint32_t> &work) {
        const size_t S = tabs.size();
        for (;;) {
            if (ci >= play.size()) return false;
            const int32_t tid = play[ci];
            const int64_t bb = ds.bed_beg[(size_t)tid], be = ds.bed_end[(size_t)tid];
            const int64_t fb = std::max<int64_t>(bb, 0), fe = all ? std::min<int64_t>(be, std::min<int64_t>(ds.lengths[(size_t)tid], (int64_t)INT32_MAX)) : INT64_MIN;
            if (!open) {
                int64_t first = INT64_MAX;
                for (size_t s = 0; s < S; ++s) {
                    const SampleTab &t = tabs[s];
                    while (run[s] < t.run_tid.size() && t.run_tid[run[s]] < tid) ++run[s];
                    if (run[s] < t.run_tid.size() && t.run_tid[run[s]] == tid) { lo[s] = hi[s] = t.run_lo[run[s]]; end[s] = t.run_lo[run[s] + 1]; first = std::min<int64_t>(first, t.pos[lo[s]]); }
                    else lo[s] = hi[s] = end[s] = 0;
                }
                t0 = (fb < fe ? fb : std::max(first, bb)) / MPT_T * MPT_T;      // (fb <= max(first, bb))
                open = true;
            }
            if (t0 >= be) { open = false; ++ci; continue; }
            bool any = false, left = false; int64_t ahead = INT64_MAX;
            for (size_t s = 0; s < S; ++s) {
                const SampleTab &t = tabs[s];
                while (lo[s] < end[s] && t.pmax[lo[s]] <= t0) ++lo[s];
                if (hi[s] < lo[s]) hi[s] = lo[s];
                while (hi[s] < end[s] && t.pos[hi[s]] < t0 + MPT_T) ++hi[s];
                any |= lo[s] < hi[s];
                if (hi[s] < end[s]) { left = true; ahead = std::min<int64_t>(ahead, t.pos[hi[s]]); }
            }
            if (!any && t0 < fe) {
                tiles.push_back(MptTile{~(int32_t)ci, (int32_t)t0, (int32_t)std::max<int64_t>(t0, fb), (int32_t)std::min<int64_t>(t0 + MPT_T, fe)});
                t0 += MPT_T;
                return true;
            }
            if (!any) {
                if (!left) { open = false; ++ci; continue; }
                t0 = ahead / MPT_T * MPT_T;                      // (ahead >= t0 + MPT_T: the position of a read no list has reached)
                continue;
            }
            work.push_back((uint32_t)tiles.size());
            tiles.push_back(MptTile{(int32_t)ci, (int32_t)t0, (int32_t)std::max<int64_t>(t0, bb), (int32_t)std::min<int64_t>(t0 + MPT_T, std::min<int64_t>(be, (int64_t)INT32_MAX))});
            for (size_t s = 0; s < S; ++s) ranges.push_back(MptRange{lo[s], hi[s]});
            t0 += MPT_T;
            return true;
        }
    }
};

int Run::format() {
    const size_t S = tabs.size();
    // ---- contigs in play: names and reference characters.  -aa: every contig of the header prints lines, reads or none
    std::vector<int32_t> play;
    if (all_level >= 2) for (size_t c = 0; c < ds->names.size(); ++c) play.push_back((int32_t)c);
    else for (const SampleTab &t : tabs) play.insert(play.end(), t.run_tid.begin(), t.run_tid.end());
    std::sort(play.begin(), play.end());
    play.erase(std::unique(play.begin(), play.end()), play.end());
    if (play.empty() || S == 0) return MSNV_OK;
    std::vector<MptContig> contigs; std::vector<char> names, ref;
    for (int32_t tid : play) {
        const std::string &nm = ds->names[(size_t)tid];
        MptContig c{ref.size(), ds->has_seq[(size_t)tid] ? (int64_t)ds->seqs[(size_t)tid].size() : -1, (uint32_t)names.size(), (uint32_t)nm.size(), ds->lengths[(size_t)tid]};
        names.insert(names.end(), nm.begin(), nm.end());
        if (c.ref_len > 0) ref.insert(ref.end(), ds->seqs[(size_t)tid].begin(), ds->seqs[(size_t)tid].end());
        contigs.push_back(c);
    }
    MptJob J{};
    MptContig *d_contigs = nullptr; char *d_names = nullptr, *d_ref = nullptr; const uint8_t **d_recs = nullptr; const MptRead **d_tabs = nullptr;
    if (int rc = up(&d_contigs, contigs)) return rc;
    if (int rc = up(&d_names, names)) return rc;
    if (int rc = up(&d_ref, ref)) return rc;
    if (int rc = up(&d_recs, d_rec)) return rc;
    if (int rc = up(&d_tabs, d_reads)) return rc;
    J.contigs = d_contigs; J.names = d_names; J.ref = d_ref; J.rec = d_recs; J.reads = d_tabs;
    J.S = (uint32_t)S; J.min_baseq = ds->params.min_baseq; J.opt = opt;

    // ---- the group's tables: at most 64 MB of cells (cnt, blen, rel; bplen with the read-offset column)
    const uint64_t cell_bytes = 12 + ((opt & MPT_BP) ? 4 : 0);
    const uint32_t G = (uint32_t)std::min<uint64_t>(2048, std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)MPT_T * S * cell_bytes)));
    J.lines_cap = G * MPT_T;
    MptTile *d_tiles = nullptr; MptRange *d_ranges = nullptr; uint32_t *d_work = nullptr; uint8_t *d_small = nullptr;
    auto table = [&](auto *&dst, uint64_t bytes) -> int {
        void *q = nullptr;
        if (int rc = alloc(&q, bytes)) return rc;
        dst = static_cast<std::remove_reference_t<decltype(dst)>>(q);
        return MSNV_OK;
    };
    if (int rc = table(d_tiles, (uint64_t)G * sizeof(MptTile))) return rc;
    if (int rc = table(d_ranges, (uint64_t)G * S * sizeof(MptRange))) return rc;
    if (int rc = table(J.cnt, (uint64_t)J.lines_cap * S * 4)) return rc;
    if (int rc = table(J.blen, (uint64_t)J.lines_cap * S * 4)) return rc;
    if (int rc = table(J.rel, (uint64_t)J.lines_cap * S * 4)) return rc;
    if (opt & MPT_BP) if (int rc = table(J.bplen, (uint64_t)J.lines_cap * S * 4)) return rc;
    if (opt & MPT_ALL) if (int rc = table(d_work, (uint64_t)G * 4)) return rc;
    if (int rc = table(J.active, (uint64_t)J.lines_cap * 4)) return rc;
    if (int rc = table(J.line_len, (uint64_t)J.lines_cap * 4)) return rc;
    if (int rc = table(J.line_off, ((uint64_t)J.lines_cap + 1) * 8)) return rc;
    if (int rc = table(J.tile_off, ((uint64_t)G + 1) * 8)) return rc;
    if (int rc = table(d_small, 32)) return rc;
    if (int rc = dev_memset(d_small, 0, 32)) return rc;
    J.tiles = d_tiles; J.ranges = d_ranges; J.work = d_work;
    J.totals = reinterpret_cast<unsigned long long *>(d_small); J.flag = reinterpret_cast<uint32_t *>(d_small + 16);
    // pinned: the group's tile offsets, and per text buffer the self-check flag as it stood behind the batch
    if (int rc = mpt_pinned_alloc(&pin_small, ((uint64_t)G + 1) * 8 + 64)) return rc;
    unsigned long long *h_tile_off = (unsigned long long *)pin_small;
    uint32_t *h_flag = (uint32_t *)((uint8_t *)pin_small + ((uint64_t)G + 1) * 8);      // [2], 16 bytes apart
    for (void *&e : ev) if (int rc = mpt_event_create(&e)) return rc;
    void **ev_start = ev, **ev_kernel = ev + 2, **ev_copy = ev + 4, *ev_m0 = ev[6], *ev_m1 = ev[7];
    if (!ctx->stream2) if (int rc = dev_stream_create(&ctx->stream2)) return rc;
    void *sa = ctx->stream, *sb = ctx->stream2;

    const uint64_t batch_bytes = knob::mptext_batch_bytes();
    char *d_text[2] = {nullptr, nullptr}; uint64_t text_cap = 0;
    struct Pending { bool on = false; int slot = 0; uint64_t bytes = 0; } pend;
    auto flush = [&]() -> int {                      // the batch in flight: wait for its copy, hand it to the sink
        if (!pend.on) return MSNV_OK;
        pend.on = false;
        if (int rc = mpt_event_wait(ev_copy[pend.slot])) return rc;
        double ms = 0;
        if (int rc = mpt_event_ms(ev_start[pend.slot], ev_kernel[pend.slot], &ms)) return rc;
        ms_write += ms;
        if (h_flag[4 * pend.slot]) return fail(MSNV_EHIP, "internal error: a cell of the mpileup text did not end where the next one starts (measure and write passes disagree)");
        return sink.put((const char *)pin_text[pend.slot], pend.bytes);
    };

    Tiler tiler(*ds, tabs, play, (opt & MPT_ALL) != 0);
    std::vector<MptTile> tiles; std::vector<MptRange> ranges; std::vector<uint32_t> work;      // work: the group's tiles that hold reads
    for (;;) {
        tiles.clear(); ranges.clear(); work.clear();
        while (tiles.size() < G && tiler.next(tiles, ranges, work)) {}
        if (tiles.empty()) break;
        const uint32_t nt = (uint32_t)tiles.size();
        if (int rc = dev_stream_wait(sa)) return rc;                       // the last group's write kernels have read its tables
        if (int rc = dev_upload(d_tiles, tiles.data(), tiles.size() * sizeof(MptTile))) return rc;
        if (int rc = dev_upload(d_ranges, ranges.data(), ranges.size() * sizeof(MptRange))) return rc;
        if (opt & MPT_ALL) if (int rc = dev_upload(d_work, work.data(), work.size() * sizeof(uint32_t))) return rc;
        if (int rc = mpt_event_record(ev_m0, sa)) return rc;
        if (int rc = mpt_measure(J, nt, (uint32_t)work.size(), sa)) return rc;
        if (int rc = mpt_event_record(ev_m1, sa)) return rc;
        if (int rc = mpt_copy_to_host_async(h_tile_off, J.tile_off, ((uint64_t)nt + 1) * 8, sa)) return rc;
        if (int rc = flush()) return rc;                                   // (the last batch's file write runs under the measure pass)
        if (int rc = dev_stream_wait(sa)) return rc;
        double ms = 0;
        if (int rc = mpt_event_ms(ev_m0, ev_m1, &ms)) return rc;
        ms_measure += ms;
        for (uint32_t i = 0; i < nt;) {
            uint32_t j = i + 1;
            while (j < nt && h_tile_off[j + 1] - h_tile_off[i] <= batch_bytes) ++j;
            const uint64_t base = h_tile_off[i], bytes = h_tile_off[j] - base;
            const uint32_t lo_t = i; i = j;
            if (!bytes) continue;
            if (bytes + 256 > text_cap) {                                  // grow both pairs of buffers: nothing may be in flight
                if (int rc = flush()) return rc;
                if (int rc = dev_stream_wait(sa)) return rc;
                if (int rc = dev_stream_wait(sb)) return rc;
                text_cap = std::max(bytes, batch_bytes) + 256;
                for (int k = 0; k < 2; ++k) {
                    mpt_pinned_free(pin_text[k]); pin_text[k] = nullptr;
                    void *q = nullptr;
                    if (int rc = alloc(&q, text_cap)) return rc;           // (the smaller one stays until the call ends)
                    d_text[k] = (char *)q;
                    if (int rc = mpt_pinned_alloc(&pin_text[k], text_cap)) return rc;
                }
            }
            const int slot = (int)(batches & 1);
            if (batches >= 2) if (int rc = mpt_stream_wait_event(sa, ev_copy[slot])) return rc;      // the copy of batch k - 2 has read this buffer
            if (int rc = mpt_event_record(ev_start[slot], sa)) return rc;
            const uint32_t w_lo = (uint32_t)(std::lower_bound(work.begin(), work.end(), lo_t) - work.begin());      // (without MPT_ALL: lo_t and j)
            const uint32_t w_hi = (uint32_t)(std::lower_bound(work.begin(), work.end(), j) - work.begin());
            if (int rc = mpt_write(J, lo_t, j, w_lo, w_hi, base, d_text[slot], sa)) return rc;
            if (int rc = mpt_event_record(ev_kernel[slot], sa)) return rc;
            if (int rc = mpt_stream_wait_event(sb, ev_kernel[slot])) return rc;
            if (int rc = mpt_copy_to_host_async(pin_text[slot], d_text[slot], bytes, sb)) return rc;
            if (int rc = mpt_copy_to_host_async(&h_flag[4 * slot], J.flag, 4, sb)) return rc;
            if (int rc = mpt_event_record(ev_copy[slot], sb)) return rc;
            if (int rc = flush()) return rc;                               // batch k - 1: its file write runs under batch k's kernel
            pend.on = true; pend.slot = slot; pend.bytes = bytes;
            ++batches;
        }
    }
    if (int rc = flush()) return rc;
    if (int rc = dev_stream_wait(sa)) return rc;
    return dev_download(totals, J.totals, sizeof totals);
}

void mpileup_params(const msnv_params *in, msnv_params &P) {      // of params only the mpileup fields are read
    msnv_params_default(&P);
    if (in) { P.min_baseq = in->min_baseq; P.flag_filter = in->flag_filter; P.count_orphans = in->count_orphans; P.max_depth = in->max_depth;
              P.min_mapq = in->min_mapq; P.ignore_overlaps = in->ignore_overlaps; }
    P.token_limit = 0;                                             // mpileup cuts nothing
}

void fill_stats(uint64_t stats[8], const Run &r, const Sink &sink) {
    if (!stats) return;
    stats[0] = r.totals[0]; stats[1] = r.tabs.size(); stats[2] = sink.n; stats[3] = r.totals[1];
    stats[4] = (uint64_t)(r.ms_measure + 0.5); stats[5] = (uint64_t)(r.ms_write + 0.5); stats[6] = r.batches; stats[7] = r.rounds;
}

}  // namespace

namespace msnv {

int mptext_records(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params, const MptBed &bed, const uint8_t *const *records,
                   const uint64_t *n_bytes, int32_t n, uint32_t opt, int32_t all_level, char **text, uint64_t *text_bytes, uint64_t stats[8]) {
    msnv_params P;
    mpileup_params(params, P);
    msnv_dataset *ds = nullptr;
    if (int rc = msnv_dataset_create(nullptr, ref, &P, &ds)) return rc;
    int rc = bed.n > 0 ? msnv_dataset_set_bed(ds, bed.n, bed.tid, bed.beg, bed.end) : MSNV_OK;
    Sink sink; sink.to_mem = true;
    if (!rc) rc = dev_set_device(ctx->device);
    if (!rc) {
        Run run(ctx, ds, sink, opt, all_level);
        const int per = knob::mptext_round_samples();
        for (int i = 0; i < n && !rc; i += per) rc = run.add_round(records + i, n_bytes + i, std::min(per, n - i), 0);
        if (!rc) rc = run.format();
        if (!rc) fill_stats(stats, run, sink);
    }
    msnv_dataset_destroy(ds);
    if (rc) return rc;
    if (!sink.mem) { sink.mem = (char *)malloc(1); if (!sink.mem) return fail(MSNV_ENOMEM, "mpileup text: out of memory"); }
    *text = sink.mem; *text_bytes = sink.n;
    sink.mem = nullptr;
    return MSNV_OK;
}

int mptext_files(msnv_ctx *ctx, const char *const *bam_paths, int32_t n_bams, const char *ref_fasta, const char *bed_path, const char *out_path,
                 int32_t host_threads, const msnv_params *params, uint32_t opt, int32_t all_level, uint64_t stats[8]) {
    msnv_params P;
    mpileup_params(params, P);
    msnv_dataset *ds = nullptr;
    if (int rc = msnv_dataset_create_from_files(nullptr, bam_paths[0], ref_fasta, &P, &ds)) return rc;
    int rc = bed_path ? msnv_dataset_set_bed_file(ds, bed_path) : MSNV_OK;
    Sink sink;
    if (!rc) {
        if (!out_path || !strcmp(out_path, "-")) sink.f = stdout;
        else { sink.f = fopen(out_path, "wb"); sink.close_f = true; if (!sink.f) rc = fail(MSNV_EIO, "cannot write %s", out_path); }
    }
    if (!rc) rc = dev_set_device(ctx->device);
    if (!rc) {
        Run run(ctx, ds, sink, opt, all_level);
        const int per = knob::mptext_round_samples();
        for (int i = 0; i < n_bams && !rc; i += per) {                  // a round of files: read and inflated by the host threads, then released
            const int m = std::min(per, n_bams - i);
            std::vector<ByteBuf> bufs((size_t)m); std::vector<uint64_t> rec_off((size_t)m, 0);
            rc = for_each_index(0, (size_t)m, pool_threads(host_threads, m), 1,
                                [&](size_t k) {
                                    BamHeader h;
                                    if (int r2 = bam_read(bam_paths[i + (int)k], h, bufs[k], rec_off[k], 1)) return r2;
                                    return check_header(*ds, h, bam_paths[i + (int)k]);
                                },
                                [&](size_t k) { return std::string(bam_paths[i + (int)k]); }, HT_READ);
            if (rc) break;
            std::vector<const uint8_t *> ptrs((size_t)m); std::vector<uint64_t> sizes((size_t)m);
            for (int k = 0; k < m; ++k) { ptrs[(size_t)k] = bufs[(size_t)k].data() + rec_off[(size_t)k]; sizes[(size_t)k] = bufs[(size_t)k].size() - rec_off[(size_t)k]; }
            rc = run.add_round(ptrs.data(), sizes.data(), m, host_threads);
        }
        if (!rc) rc = run.format();
        if (!rc && fflush(sink.f) != 0) rc = fail(MSNV_EIO, "mpileup text: write failed");
        if (!rc) fill_stats(stats, run, sink);
    }
    msnv_dataset_destroy(ds);
    return rc;
}

}  // namespace msnv

namespace {

// opts (NULL: none) as the kernels' option bits and the -a level
int read_opts(const char *who, const msnv_mpileup_text_opts *o, uint32_t &opt, int32_t &all_level) {
    opt = 0; all_level = 0;
    if (!o) return MSNV_OK;
    if (o->all_positions < 0 || o->all_positions > 2) return fail(MSNV_EINVAL, "%s: all_positions is %d, not 0, 1 (-a) or 2 (-aa)", who, o->all_positions);
    if (o->reserved != 0) return fail(MSNV_EINVAL, "%s: the reserved field of msnv_mpileup_text_opts is %d, not 0", who, o->reserved);
    all_level = o->all_positions;
    opt = (all_level ? MPT_ALL : 0u) | (o->output_mq ? MPT_MQ : 0u) | (o->output_bp ? MPT_BP : 0u);
    return MSNV_OK;
}

}  // namespace

extern "C" void msnv_mpileup_text_opts_default(msnv_mpileup_text_opts *o) { if (o) *o = msnv_mpileup_text_opts{0, 0, 0, 0}; }

extern "C" int msnv_mpileup_text_ex(msnv_ctx *ctx, const msnv_mpileup_text_args *a, const msnv_mpileup_text_opts *opts, uint64_t stats[8]) {
    clear_error();
    if (!ctx || !a || !a->bam_paths || a->n_bams <= 0) return fail(MSNV_EINVAL, "msnv_mpileup_text: ctx and bam_paths are required");
    for (int i = 0; i < a->n_bams; ++i) if (!a->bam_paths[i]) return fail(MSNV_EINVAL, "msnv_mpileup_text: BAM path %d is NULL", i);
    uint32_t opt; int32_t lvl;
    if (int rc = read_opts("msnv_mpileup_text_ex", opts, opt, lvl)) return rc;
    try { return mptext_files(ctx, a->bam_paths, a->n_bams, a->ref_fasta, a->bed_split_path, a->out_path, a->host_threads, &a->params, opt, lvl, stats); }
    catch (const std::exception &e) { return fail(MSNV_ENOMEM, "msnv_mpileup_text: %s", e.what()); }
}

extern "C" int msnv_mpileup_text(msnv_ctx *ctx, const msnv_mpileup_text_args *a, uint64_t stats[8]) { return msnv_mpileup_text_ex(ctx, a, nullptr, stats); }

extern "C" int msnv_mpileup_text_records_ex(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params, const msnv_mpileup_text_opts *opts, int32_t n_bed,
                                            const int32_t *bed_tid, const int64_t *bed_beg, const int64_t *bed_end, const uint8_t *const *records,
                                            const uint64_t *n_bytes, int32_t n, char **text, uint64_t *text_bytes, uint64_t stats[8]) {
    clear_error();
    if (!ctx || !ref || !text || !text_bytes || n < 0 || (n && (!records || !n_bytes)) || n_bed < 0 || (n_bed && (!bed_tid || !bed_beg || !bed_end)))
        return fail(MSNV_EINVAL, "msnv_mpileup_text_records: bad argument");
    for (int i = 0; i < n; ++i) if (n_bytes[i] && !records[i]) return fail(MSNV_EINVAL, "msnv_mpileup_text_records: stream %d is NULL", i);
    *text = nullptr; *text_bytes = 0;
    uint32_t opt; int32_t lvl;
    if (int rc = read_opts("msnv_mpileup_text_records_ex", opts, opt, lvl)) return rc;
    try { return mptext_records(ctx, ref, params, MptBed{n_bed, bed_tid, bed_beg, bed_end}, records, n_bytes, n, opt, lvl, text, text_bytes, stats); }
    catch (const std::exception &e) { return fail(MSNV_ENOMEM, "msnv_mpileup_text_records: %s", e.what()); }
}

extern "C" int msnv_mpileup_text_records(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params, int32_t n_bed, const int32_t *bed_tid,
                                         const int64_t *bed_beg, const int64_t *bed_end, const uint8_t *const *records, const uint64_t *n_bytes, int32_t n,
                                         char **text, uint64_t *text_bytes, uint64_t stats[8]) {
    return msnv_mpileup_text_records_ex(ctx, ref, params, nullptr, n_bed, bed_tid, bed_beg, bed_end, records, n_bytes, n, text, text_bytes, stats);
}

extern "C" void msnv_mpileup_text_geometry(int32_t *tile_positions, int32_t *lds_reads) {
    if (tile_positions) *tile_positions = MPT_T;
    if (lds_reads) *lds_reads = MPT_B;
}
