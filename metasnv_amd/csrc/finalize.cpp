// metasnv_amd/csrc/finalize.cpp -- a dataset's samples -> its tile index and device columns: every table the pileup, gate, gather and
// coverage kernels read (device.h: DeviceCols).  finalize_dataset is a short driver over struct Finalize, whose member functions are the
// stages in the order they run; where a stage has a host form (loops over the samples' staging, pack.cpp's output) and a device form
// (devfin_* in devfin.hip, for datasets whose samples were all packed on the device), it picks by Finalize::R at its top.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <mutex>
#include <thread>

#include "device.h"
#include "devfin.h"
#include "devpack.h"
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

namespace msnv {
// The device's quality column (kernels.hip: lowq_fetch): bit i = quality byte i of the host staging is below the cutoff.  The staged
// bytes are clamped to <= 127 (pack_sample), padding bytes are 0 (flagged unless the cutoff is 0; the kernels mask what lies beyond a piece).
static void pack_lowq(const uint8_t *q, size_t n, int cutoff, std::vector<uint8_t> &out) {
    out.assign((n + 7) / 8, 0);
    // staged bytes are 0 .. 127, or 0x80 for a base behind snpCall's token limit: as SIGNED bytes that one is below every cutoff,
    // the cutoff 0 (mpileup -Q 0: no quality is too low) included
    const int c_eff = std::min(std::max(cutoff, -127), 127);
    const bool all = cutoff > 127;
    size_t i = 0;
#if defined(__SSE2__)
    const __m128i c = _mm_set1_epi8((char)c_eff);
    for (; i + 16 <= n; i += 16) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(q + i));
        const uint32_t m = all ? 0xffffu : (uint32_t)_mm_movemask_epi8(_mm_cmpgt_epi8(c, v));
        out[i >> 3] = (uint8_t)m; out[(i >> 3) + 1] = (uint8_t)(m >> 8);
    }
#endif
    for (; i < n; ++i) if (all || (int)(int8_t)q[i] < c_eff) out[i >> 3] |= (uint8_t)(1u << (i & 7));
}

// Layout of the narrow path: padded per-piece columns (msnv_pileup_tiles_narrow32) or the dense block stream
// (msnv_pileup_tiles_dense: no alignment padding, every lane owns 32 real bases, but up to two segments per block).
// Dense wins for short pieces (50-base reads: -18 % kernel time), loses from ~100 bases on (kernels.hip), so the
// dataset picks it when the mean piece is shorter than 62 bases.  MSNV_LAYOUT=pieces|dense overrides.
static bool layout_dense(uint64_t n_pieces, uint64_t n_bases) {
    if (const char forced = knob::layout()) return forced == 'd';
    return n_pieces && n_bases / n_pieces < 62;      // (round 3, one bit of quality per base, eight workgroups per CU: 50-base reads 0.589 vs 0.535 ms, 75-base reads 0.476 vs 0.535 -- break-even near 62; it was 72: profiles/r03zap_layout_by_read_length.txt)
}

// A (contig, tile) run of one sample whose depth can reach NARROW_MAX_DEPTH does not fit the byte bins of the narrow
// kernels, and the kernels slow down well before that (8 samples at ~100x: 0.531 ms unsplit, 0.336 ms when runs deeper than
// 192 are dealt into groups of <= 128; at ~400x 2.68 ms with groups of 240, 1.66 ms with groups of 128).  Instead of a second kernel with wider bins, the run is dealt into groups of pieces that each stay below the
// limit (round robin in start order, verified with an exact sweep, more groups if needed); every group becomes its own
// (sample, tile) pair and the per-sample results are summed on the device (gather / scatter accumulate).  The pieces of a
// group are made contiguous -- headers AND bases / qualities (MSNV_DEEP_RELOCATE=0 leaves the columns in read order: every group's
// workgroups then fetch almost every cache line of the run).  MSNV_DEEP=wide keeps such runs whole for msnv_pileup_tiles_wide instead.
// MSNV_SPLIT_AT and MSNV_GROUP_DEPTH move the two depths; all three are read per dataset (knobs.h).
static bool deep_runs_split() { return !knob::deep_wide(); }
static uint32_t deep_split_at() { return knob::split_at((int)NARROW_MAX_DEPTH); }
static int split_deep_runs(SampleCols &sc, int device) {
    const size_t n = sc.hdr.size();
    sc.grp.assign(n, 0);
    if (!deep_runs_split()) return MSNV_OK;
    struct Ev { uint32_t pos; int32_t delta; uint32_t g; };
    std::vector<Ev> ev;
    std::vector<uint32_t> cur, mx, order;
    bool any_split = false;
    const uint32_t split_at = deep_split_at(), group_depth = knob::group_depth();
    size_t i = 0;
    while (i < n) {
        size_t j = i;
        while (j < n && sc.tid[j] == sc.tid[i] && sc.hdr[j].gpos / TILE == sc.hdr[i].gpos / TILE) ++j;
        uint32_t bound = 0;
        for (size_t k = i; k < j; ++k) bound = std::max<uint32_t>(bound, sc.depth[k]);
        if (bound >= split_at) {
            const size_t m = j - i;
            auto sweep = [&](uint32_t G) -> uint32_t {            // largest per-position depth of any group
                ev.clear();
                for (size_t k = 0; k < m; ++k) {
                    const ReadHdr &h = sc.hdr[i + k];
                    ev.push_back(Ev{h.gpos, +1, (uint32_t)(k % G)});
                    ev.push_back(Ev{h.gpos + h.cig, -1, (uint32_t)(k % G)});
                }
                std::sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) { return a.pos != b.pos ? a.pos < b.pos : a.delta < b.delta; });
                cur.assign(G, 0); mx.assign(G, 0);
                for (const Ev &e : ev) { cur[e.g] += (uint32_t)e.delta; mx[e.g] = std::max(mx[e.g], cur[e.g]); }
                return *std::max_element(mx.begin(), mx.end());
            };
            const uint32_t exact = sweep(1);
            if (exact < split_at) {
                for (size_t k = i; k < j; ++k) sc.depth[k] = (uint16_t)exact;        // the start-time bound was pessimistic
            } else {
                uint32_t G = exact / group_depth + 1;
                while (sweep(G) >= NARROW_MAX_DEPTH) ++G;
                std::vector<uint32_t> gmax = mx;
                order.resize(m);
                for (size_t k = 0; k < m; ++k) order[k] = (uint32_t)k;
                std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return a % G < b % G; });
                std::vector<ReadHdr> h2(m); std::vector<int32_t> t2(m), e2(m);
                for (size_t k = 0; k < m; ++k) { h2[k] = sc.hdr[i + order[k]]; t2[k] = sc.tid[i + order[k]]; e2[k] = sc.end[i + order[k]]; }
                for (size_t k = 0; k < m; ++k) {
                    sc.hdr[i + k] = h2[k]; sc.tid[i + k] = t2[k]; sc.end[i + k] = e2[k];
                    sc.grp[i + k] = (uint16_t)(1 + order[k] % G);
                    sc.depth[i + k] = (uint16_t)gmax[order[k] % G];
                }
                any_split = true;
            }
        }
        i = j;
    }
    // The bases and qualities follow their headers: a group's pieces were every G-th piece of the run in memory, so the workgroups
    // of the G groups -- at G different times -- each fetched (almost) every cache line of the run (one sample at 1600x: 6.2 GB of
    // HBM reads per pass for 2.2 GB of columns).  Same pieces (bases + twice as many quality bytes, alignment padding included), new order.
    if (any_split && !knob::deep_relocate_off()) {
        if (sc.on_device) {                              // (the relocation still runs on host staging: a device-packed sample comes back for it)
            if (int rc = dev_set_device(device)) return rc;
            if (int rc = devpack_sample_to_host(sc)) return rc;
        }
        std::vector<uint8_t> nseq(sc.seq.size(), 0xff), nqual(sc.qual.size(), 0);
        size_t so = 0;
        auto stored = [](uint32_t bases) { return (size_t)(((bases + 1u) / 2u + SEQ_ALIGN - 1u) & ~(SEQ_ALIGN - 1u)); };      // seq bytes of a piece with its alignment padding (pack_sample)
        for (size_t k = 0; k < n; ++k) {
            const size_t blk = stored(sc.hdr[k].cig);
            if (so + blk > nseq.size() || 2 * (so + blk) > nqual.size()) return MSNV_OK;       // (cannot happen: the blocks are a permutation; keep the old layout rather than write past the end)
            memcpy(nseq.data() + so, sc.seq.data() + sc.hdr[k].seqoff, blk);
            memcpy(nqual.data() + 2 * so, sc.qual.data() + 2 * (size_t)sc.hdr[k].seqoff, 2 * blk);
            so += blk;
        }
        so = 0;
        for (size_t k = 0; k < n; ++k) { sc.hdr[k].seqoff = (uint32_t)so; so += stored(sc.hdr[k].cig); }
        sc.seq.swap(nseq); sc.qual.swap(nqual);
    }
    return MSNV_OK;
}

// Rewrites seq / qual of one sample into the dense block streams (dataset.h) and fills blk / run_*.
// hdr must already be grouped by (contig, tile); hdr[i].gpos is still contig-relative (contigs start on tile boundaries).
static void relayout_dense(SampleCols &sc) {
    const size_t n = sc.hdr.size();
    std::vector<uint8_t> nseq, nqual;
    nseq.reserve(sc.seq.size()); nqual.reserve(sc.qual.size());
    sc.blk.clear(); sc.run_blk_lo.clear(); sc.run_nblk.clear(); sc.run_seq0.clear();
    size_t i = 0;
    while (i < n) {
        size_t j = i;
        while (j < n && sc.tid[j] == sc.tid[i] && sc.hdr[j].gpos / TILE == sc.hdr[i].gpos / TILE && sc.grp[j] == sc.grp[i]) ++j;
        const uint32_t blk0 = (uint32_t)sc.blk.size();
        const size_t seq0 = nseq.size();                       // multiple of 16 bytes
        uint64_t cursor = 0;                                   // bases from the start of this run's stream
        auto block = [&](uint64_t b) -> uint32_t & {
            while (sc.blk.size() <= blk0 + b) sc.blk.push_back(BLK_EMPTY);
            return sc.blk[blk0 + b];
        };
        for (size_t k = i; k < j; ++k) {
            ReadHdr &h = sc.hdr[k];
            const uint32_t len = h.cig, P = h.gpos % TILE;
            cursor = (cursor + 1) & ~1ull;
            uint64_t b = cursor / 32; uint32_t o = (uint32_t)(cursor % 32);
            if (o != 0) {
                const uint32_t cur = block(b);
                const bool has_b = ((cur >> 17) & 0xfffu) != BLK_NO_B;
                if (has_b || len < 32 - o) { cursor = (b + 1) * 32; ++b; o = 0; }      // a second head, or one that ends inside the block: fresh block
            }
            // copy the piece: seq nibbles are byte aligned at both ends (even cursor), qualities 1:1
            const size_t so = seq0 + cursor / 2, qo = 2 * seq0 + cursor;
            if (nseq.size() < so + (len + 1) / 2) nseq.resize(so + (len + 1) / 2, 0xff);
            if (nqual.size() < qo + len) nqual.resize(qo + len, 0);
            memcpy(nseq.data() + so, sc.seq.data() + h.seqoff, (len + 1) / 2);
            if (len & 1u) nseq[so + len / 2] |= 0xf0;           // the pad nibble of an odd piece reads as N
            memcpy(nqual.data() + qo, sc.qual.data() + 2 * (size_t)h.seqoff, len);
            h.seqoff = (uint32_t)so;                           // (sample-relative; the wide kernel reads pieces through it)
            // descriptors
            uint32_t done = 0;
            if (o != 0) {                                      // head of the piece = segment B of block b
                uint32_t &w = block(b);
                w = (w & ~(0xfffu << 17)) | ((P - o + 32u) << 17);
                done = 32 - o;
                if (done == len) w |= BLK_END_B;
                ++b;
            }
            bool first = (o == 0);
            while (done < len) {
                const uint32_t na = std::min<uint32_t>(32, len - done);
                uint32_t &w = block(b);
                w = (w & (0xfffu << 17)) | (P + done) | na << 11 | (first ? BLK_START_A : 0u) | (done + na == len ? BLK_END_A : 0u);
                first = false; done += na; ++b;
            }
            cursor += len;
        }
        const uint32_t nb = (uint32_t)sc.blk.size() - blk0;
        nseq.resize(seq0 + (size_t)nb * 16, 0xff);
        nqual.resize(2 * seq0 + (size_t)nb * 32, 0);
        sc.run_blk_lo.push_back(blk0); sc.run_nblk.push_back(nb); sc.run_seq0.push_back((uint32_t)seq0);
        i = j;
    }
    sc.seq.swap(nseq); sc.qual.swap(nqual);
}

// Index loops of finalize that run per sample (16 M pieces on the benchmark shape, 6e8 at BASELINE configs[2] scale): dealt to host threads.
template <typename F>
static void parallel_for(size_t n, F fn) {
    const unsigned hw = msnv_default_threads();
    const size_t nt = std::min<size_t>(std::min<size_t>(n, hw), 64);
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) fn(i); return; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back([&]() { for (;;) { const size_t i = next.fetch_add(1); if (i >= n) break; fn(i); } });
    for (auto &t : th) t.join();
}

// The index tables of a dataset go up TOGETHER: finalize_dataset builds some thirty small tables (pairs, work items, tile tables, gate
// descriptors ...); an allocation and a synchronous copy each was a millisecond of finalize.  add() copies a table into one staging block,
// commit() makes one allocation and one copy of everything added so far and sets the tables' device pointers (so nothing on the device may
// use a table between its add() and the next commit()).  The block is owned by DeviceCols::blocks.  With guarded allocations
// (MSNV_GUARD_ALLOC=1) every table keeps an allocation of its own, so that a read past its end still faults.
struct TableArena {
    struct Ent { void **dst; size_t off, bytes; };
    std::vector<Ent> ents;
    std::vector<uint8_t> stage;
    template <typename T>
    int add(T **dst, const std::vector<T> &v, size_t pad_elems = 0) {
        const size_t off = (stage.size() + 255) & ~(size_t)255, bytes = (v.size() + pad_elems) * sizeof(T);
        stage.resize(off + std::max<size_t>(bytes, 16), 0);
        if (!v.empty()) memcpy(stage.data() + off, v.data(), v.size() * sizeof(T));
        ents.push_back(Ent{reinterpret_cast<void **>(dst), off, std::max<size_t>(bytes, 16)});
        return MSNV_OK;
    }
    int commit(DeviceCols &d) {
        if (ents.empty()) return MSNV_OK;
        const bool guard = knob::guard_alloc();
        if (guard) {
            for (const Ent &e : ents) {
                if (int rc = dev_alloc(e.dst, e.bytes, &d.device_bytes)) return rc;
                if (int rc = dev_upload(*e.dst, stage.data() + e.off, e.bytes)) return rc;
            }
        } else {
            void *block = nullptr;
            if (int rc = dev_alloc(&block, stage.size() + 256, &d.device_bytes)) return rc;
            d.blocks.emplace_back(block, stage.size() + 256);
            if (int rc = dev_upload(block, stage.data(), stage.size())) return rc;
            for (const Ent &e : ents) *e.dst = static_cast<uint8_t *>(block) + e.off;
        }
        ents.clear(); stage.clear();
        return MSNV_OK;
    }
};

namespace {
// Everything one call of finalize_dataset works on.  The stages are member functions, declared in the order finalize_dataset calls them; each
// says what it takes and what it leaves.  The members stand under the stage that fills them; later stages only read them unless they say
// otherwise.  Host words that an asynchronous copy or the coverage tables' helper thread touches are members, never a stage's locals.
struct Finalize {
    // ---- the inputs, and what every stage reads
    msnv_dataset &ds; const size_t S, NC;
    const int device; void *const stream;                           // the context's (a dataset without one: device 0, the null stream)
    DeviceCols *d = nullptr;                                        // tile_layout(): ds.dev
    TableArena arena, cov_arena;                                    // the index tables (upload_index() commits them) / the coverage index's (coverage_index_up())
    // ---- decide_route(), and the three flags that follow from it where the layout is known
    struct Route {
        // Device-packed samples (devpack.hip) keep their piece headers and intervals in HBM.  When every sample is one, the per-piece and
        // per-interval loops run there as kernels (devfin_* in devfin.hip) and the host works on (sample, tile) pairs only.  Mixed datasets
        // take the host loops: the headers come down first (MSNV_FINALIZE=host forces that; tests compare the two).
        bool fast = false;
        // layout_samples(): the dense block layout of short pieces (layout_dense), decided behind the host's deep-run split
        bool dense = false;
        // narrow_chunks(): fast, piece layout -- the pieces are in HBM: the chunks of every narrow pair are cut there by a kernel that runs the
        // same greedy rule as the host's loop, the work items learn their ranges there too
        bool chunks_on_device = false;
        // columns(): fast, piece layout -- every sample's columns are in the rounds' buffers, already in this layout (devpack_place_columns)
        bool cols_on_device = false;
    } R;
    // ---- tile_layout()
    std::vector<int64_t> maxend;                                    // per contig: its length or the furthest read end (0: not selected)
    uint64_t nt = 0, npos = 0;                                      // tiles, positions (nt * TILE)
    // ---- reference(), callable_ranges()
    std::vector<uint32_t> ref4, vb_host, ve_host;
    // ---- layout_samples(): first piece / seq byte / dense block of every sample (S + 1)
    std::vector<uint64_t> rbase, sbase, bbase;
    // ---- pairs_per_sample()
    struct PairTmp { uint32_t tile, sample, lo, hi, maxd, run, grp; };
    std::vector<std::vector<PairTmp>> per_sample;
    uint64_t tot_reads = 0, tot_pile_reads = 0, tot_bases = 0;
    // ---- pair_csr(), pair_classes()
    std::vector<uint32_t> tps, tpm;                                 // per tile: first pair, first merged pair
    std::vector<TilePair> pairs;                                    // (slots() puts the slot into TilePair::pad)
    std::vector<uint8_t> fuse_tile;                                 // tiles piled up by ONE whole-tile work item (work_list(): 2 = of one pair)
    // ---- work_list(); partial_rows() fills slot and part_*, the chunk stages chunk_* and first
    std::vector<WorkItem> work;
    struct MergedGroup { uint32_t pair_lo, pair_hi, tile; };
    std::vector<MergedGroup> groups;                                // in work-item order
    // ---- merged_chunks(), narrow_chunks().  Layout of d->chunks (round 6): the merged groups' chunks FIRST -- their number is the host's --, the
    // narrow work items' behind them: on the fast path those are cut in HBM and nobody waits for their count (devfin_chunks_launch).
    std::vector<ChunkDesc> mchunks, nchunks;                        // merged groups' / narrow items' (host loops only)
    std::vector<PieceHdr> hm;
    std::vector<DevMergedSrc> hm_src;                               // fast: the pairs whose headers a kernel writes
    uint64_t hm_count = 0, M = 0;                                   // M: the merged groups' chunks
    std::vector<MergedGroupDev> mgroups;
    std::vector<std::vector<uint32_t>> hdr4_of;                     // 4-byte piece headers, per sample (chunk-relative offsets: filled with the chunks)
    std::vector<uint32_t> narrow_pairs, item_first;                 // fast, piece layout: the narrow items' pairs in item order; every item's first entry
    uint64_t chunk_cap = 0;                                         // ... and the room their chunks get
    // ---- upload_index()
    uint64_t chunk_room = 0;                                        // descriptors d->chunks has room for
    // ---- columns(): what its upload threads share
    std::atomic<size_t> up_next{0}; std::atomic<int> up_err{0}; std::mutex up_mu; std::string up_msg;
    std::vector<uint8_t> on_dev;                                    // per sample: packed on the device (devpack_fill_padding)
    // ---- launch_coverage(): the coverage tables on a thread of their own (MSNV_COV_THREAD=1).  The last member: joined before any other goes.
    ThreadJob cov_job;

    explicit Finalize(msnv_dataset &ds_) : ds(ds_), S(ds_.samples.size()), NC(ds_.names.size()), device(ds_.ctx ? ds_.ctx->device : 0), stream(ds_.ctx ? ds_.ctx->stream : nullptr) {}

    // Takes: the samples as the per-read stage left them.  Leaves: R.fast (the deep runs dealt by devfin_deep_runs where there are any); for a
    // device-packed dataset that takes the host loops, its pieces and intervals as host staging.
    int decide_route();
    // Takes: the samples' furthest ends (host loops or devfin_overhang).  Leaves: maxend, ds.tile_base / tile_contig / n_tiles, nt, npos, d.
    int tile_layout();
    // Takes: the tile layout, R.fast, d: ALL that coverage_tables() reads.  Leaves: the coverage index's kernels queued (fast) and, with
    // MSNV_COV_THREAD=1, coverage_tables() running on cov_job's thread.
    int launch_coverage();
    // The genome coverage index into A.  Writes d->n_cov_*, d->n_contigs, d->n_cov_work_wide and ds.cov_row_*, which no other stage touches
    // until coverage_index_up() has joined.  coverage_runs_host / coverage_pairs_host: its host loops.
    struct CP { uint32_t tile, sample, lo, hi; };                   // intervals [lo, hi) of `sample` may touch `tile`
    int coverage_tables(TableArena &A, bool in_thread);
    void coverage_runs_host(std::vector<Pair32> &iv, std::vector<uint64_t> &cvbase, std::vector<CP> &flat);
    int coverage_pairs_host(const std::vector<CP> &flat, const std::vector<uint64_t> &cvbase, std::vector<TilePair> &cpairs, std::vector<WorkItem> &cwork, bool in_thread);
    // Leaves: ref4 (nt16 codes) and the lower-case bits in the arena, ds.info.bytes_ref.
    int reference();
    // Leaves: vb_host / ve_host, the callable range inside every tile, and their tables in the arena.
    int callable_ranges();
    // Takes: R.fast.  Leaves: the deep runs of host staging dealt into groups, THEN R.dense, the dense streams (devfin_dense or the host
    // re-layout) where it holds, rbase / sbase / bbase.
    int layout_samples();
    // Leaves: per_sample (a sample's (tile, group) runs of pieces), linear positions and the padding fill in host staging, the totals,
    // ds.first_tid / first_pos.
    int pairs_per_sample();
    // Takes: per_sample.  Leaves: tps, pairs (sample order inside a tile).
    int pair_csr();
    // Leaves: fuse_tile, TilePair::pad = 2 for the pairs of merged groups, every tile's pairs in class order, tpm.
    int pair_classes();
    // Leaves: ds.tile_slot_base / tile_slot_stride / slot_sample, TilePair::pad = kind | slot << 8, d->tile_nslots in the arena.
    int slots();
    // Leaves: work (narrow items, merged items with the whole-tile ones last, wide items), groups, d->n_work_* and d->n_groups_solo.
    int work_list();
    // Leaves: WorkItem::slot / part_lo / part_hi, the active, gather and gate tile tables in the arena, d->part_bytes, wide_tot, use_dirty.
    int partial_rows();
    // Leaves: mchunks, mgroups, M, the merged items' chunk ranges; the merged headers (hm) or, fast, their sources (hm_src, hm_count).
    int merged_chunks();
    // Leaves: R.chunks_on_device; the narrow items' chunks and 4-byte headers (host cut: nchunks, hdr4_of, WorkItem::first) or what the device's
    // cut needs (narrow_pairs, item_first, chunk_cap).
    int narrow_chunks();
    int narrow_chunks_host();
    // Takes: every table added to the arena so far.  Leaves: them in HBM (one commit), d->chunks with the host's share; fast: the kernels that
    // finish chunks, merged headers, WorkItem::first and the 16-byte headers queued, none waited for.
    int upload_index();
    // Leaves: R.cols_on_device, the samples' columns in the dataset's (uploaded, copied or adopted), the padding pass where it is needed,
    // ds.info.bytes_*.  upload_columns: one of its upload threads.
    int columns();
    void upload_columns();
    // Leaves: the allele bookkeeping picked (planes or events), the per-pass buffers allocated, ds.info's counts.
    int intermediates();
    // Takes: cov_job running, or nothing yet.  Leaves: the coverage tables built (joined or inline), in HBM, the accumulators allocated.
    int coverage_index_up();
    // Finalize's last wait.  Leaves: d->n_chunks (the table cut again with the exact count where it overflowed), the pack's tables released,
    // ds.info.bytes_index / device_bytes, ds.finalized.
    int last_wait();
};

int Finalize::decide_route() {
    bool any_dev = false, all_dev = true;
    for (const SampleCols &sc : ds.samples) { any_dev |= sc.dev_index; all_dev &= sc.dev_index; }
    R.fast = any_dev && all_dev && HDR4 && deep_runs_split();
    if (knob::finalize_on_host()) R.fast = false;
    if (R.fast) {
        uint64_t np = 0, nb = 0;
        for (const SampleCols &sc : ds.samples) { np += sc.n_dev_pieces; nb += sc.n_pileup_bases; }
        if (layout_dense(np, nb) && knob::dense_relayout_on_host()) R.fast = false;      // (the dense re-layout on host staging: tests compare the two)
        // deep (sample, tile) runs: their exact depth, and -- where a run really is that deep -- its pieces dealt into groups and the sample's
        // columns re-laid, by kernels (devfin.hip: devfin_deep_runs; MSNV_DEEP_RELOCATE=0, a host-only experiment, takes the host loops)
        const uint32_t split_at = deep_split_at();
        bool any_deep = false;
        for (const SampleCols &sc : ds.samples) for (const DevPair &p : sc.dev_pairs) if (p.maxd >= split_at) { any_deep = true; break; }
        if (R.fast && any_deep) {
            if (knob::deep_relocate_off()) R.fast = false;
            else {
                bool fallback = false;
                if (int rc = devfin_deep_runs(ds, split_at, knob::group_depth(), &fallback)) return rc;
                if (fallback) R.fast = false;
            }
        }
    }
    if (any_dev && !R.fast) { if (int rc = devpack_sync_pending(ds)) return rc; if (int rc = devpack_download_pieces(ds)) return rc; }
    fin_trace("decide / download");
    return MSNV_OK;
}

// ---- tile layout: every selected contig owns ceil(max(L, furthest read end) / TILE) tiles
int Finalize::tile_layout() {
    maxend.assign(NC, 0);
    for (size_t c = 0; c < NC; ++c) maxend[c] = ds.sel[c] ? ds.lengths[c] : 0;
    if (!R.fast) {       // (fast: the pieces are in HBM -- devfin_overhang below; qaCompute's intervals never reach beyond a contig's length)
        // per sample: the contigs it touches and how far (reads are sorted by contig: runs), merged under a lock
        std::mutex mu;
        parallel_for(S, [&](size_t s) {
            const SampleCols &sc = ds.samples[s];
            std::vector<std::pair<int32_t, int64_t>> mine;
            for (size_t i = 0; i < sc.hdr.size(); ++i) {
                if (mine.empty() || mine.back().first != sc.tid[i]) mine.emplace_back(sc.tid[i], 0);
                mine.back().second = std::max<int64_t>(mine.back().second, sc.end[i]);
            }
            for (size_t i = 0; i < sc.cov_tid.size(); ++i) {
                if (!ds.sel[(size_t)sc.cov_tid[i]]) continue;
                if (mine.empty() || mine.back().first != sc.cov_tid[i]) mine.emplace_back(sc.cov_tid[i], 0);
                mine.back().second = std::max<int64_t>(mine.back().second, std::min<int64_t>((int64_t)sc.cov_beg[i] + 1, ds.lengths[(size_t)sc.cov_tid[i]]));
            }
            std::lock_guard<std::mutex> lk(mu);
            for (const auto &m : mine) maxend[(size_t)m.first] = std::max(maxend[(size_t)m.first], m.second);
        });
    }
    fin_trace("  maxend loops");
    if (R.fast) if (int rc = devfin_overhang(ds, maxend)) return rc;       // (reads that run past their contig: from the device's per-contig maxima)
    fin_trace("  devfin_overhang");
    ds.tile_base.assign(NC, UINT32_MAX);
    ds.tile_contig.clear();
    nt = 0;
    for (size_t c = 0; c < NC; ++c) {
        if (!ds.sel[c]) continue;
        ds.tile_base[c] = (uint32_t)nt;
        uint64_t n = ((uint64_t)maxend[c] + TILE - 1) / TILE;
        for (uint64_t k = 0; k < n; ++k) ds.tile_contig.push_back((uint32_t)c);
        nt += n;
        if (nt * TILE >= 0xffffffffull) return fail(MSNV_EDOMAIN, "shard spans more than 2^32 positions: shard the contigs further");
    }
    ds.n_tiles = (uint32_t)nt;
    npos = nt * TILE;

    fin_trace("  tile tables");
    d = new DeviceCols();
    ds.dev = d;
    d->n_tiles = ds.n_tiles; d->n_samples = (uint32_t)S;
    return MSNV_OK;
}

int Finalize::launch_coverage() {
    if (R.fast) if (int rc = devfin_coverage_launch(ds, *d)) return rc;     // (the coverage index's kernels go first: they run while the host builds the pair tables)
    if (R.fast && ds.dp.fin.cov_launched && knob::cov_thread()) {
        cov_job.th = std::thread([this]() {
            (void)dev_set_device(device);
            try { cov_job.rc = coverage_tables(cov_arena, true); } catch (const std::exception &e) { cov_job.rc = fail_quiet(MSNV_ENOMEM, "coverage index: %s", e.what()); }
            if (cov_job.rc) cov_job.msg = msnv_last_error();
        });
    }
    fin_trace("tile layout");
    return MSNV_OK;
}

// ---- genome coverage index: intervals of qaCompute's difference array, grouped by tile.  The host's share -- pair tables by tile, accumulator
// rows, work items (0.5 ms of loops on the benchmark shape) -- needs the index's kernels' results and nothing else of finalize.  On a thread
// of its own beside the tile index (MSNV_COV_THREAD=1) it made finalize SLOWER (median of twelve builds 2.9-3.3 ms against 2.3: the thread's
// start and wake-up cost more than the loops; profiles/r06_variants.txt): it runs behind the wait for those kernels, on this thread.
int Finalize::coverage_tables(TableArena &A, bool in_thread) {
    std::vector<Pair32> iv;
    std::vector<uint64_t> cvbase(S + 1, 0);
    std::vector<CP> flat;                                        // all samples' (tile, sample) runs, sample after sample, tiles ascending inside a sample
    bool tables_on_device = false;                               // (round 6: devfin_coverage has cut the pair tables, the rows and the work items in HBM)
    if (R.fast) {
        // the intervals are in HBM: filtered, made linear and grouped by (sample, tile) there (devfin.hip: devfin_coverage); the runs come
        // back sample-major with the tiles ascending, which is the order the loops below want
        std::vector<DevCovPair> cp;
        if (int rc = devfin_coverage(ds, *d, cvbase, cp)) return rc;
        if (!in_thread) fin_trace("  devfin_coverage");
        tables_on_device = ds.dp.fin.cov_tables_done;
        flat.resize(cp.size());
        bool ordered = true;
        for (size_t i = 0; i < cp.size(); ++i) {
            flat[i] = CP{cp[i].tile, cp[i].sample, cp[i].lo, cp[i].hi};
            if (i && (cp[i].sample < cp[i - 1].sample || (cp[i].sample == cp[i - 1].sample && cp[i].tile < cp[i - 1].tile))) ordered = false;
        }
        if (!ordered) std::stable_sort(flat.begin(), flat.end(), [](const CP &a, const CP &b) { return a.sample != b.sample ? a.sample < b.sample : a.tile < b.tile; });
    }
    else coverage_runs_host(iv, cvbase, flat);
    std::vector<TilePair> cpairs;
    std::vector<WorkItem> cwork;
    if (!tables_on_device) if (int rc = coverage_pairs_host(flat, cvbase, cpairs, cwork, in_thread)) return rc;
    std::vector<uint32_t> tlen(nt + 1, 0), tcont(nt + 1, 0);
    for (uint64_t t = 0; t < nt; ++t) {
        const size_t c = ds.tile_contig[t];
        const int64_t t0 = (int64_t)(t - ds.tile_base[c]) * TILE;
        tlen[t] = (uint32_t)std::min<int64_t>(std::max<int64_t>(ds.lengths[c] - t0, 0), TILE);
        tcont[t] = (uint32_t)c;
    }
    if (!R.fast) d->n_cov_iv = iv.size();
    for (int k = 0; k < 4; ++k) iv.push_back(Pair32{0u, 0u});     // behind the last interval: what the idle lanes of msnv_coverage_tiles load, four at a time (they touch nothing)
    d->n_contigs = (uint32_t)NC;
    if (!R.fast) if (int rc = A.add(&d->cov_iv, iv, 1)) return rc;
    if (int rc = A.add(&d->s_cov_base, cvbase)) return rc;
    if (!tables_on_device) {
        if (int rc = A.add(&d->cov_pairs, cpairs, 1)) return rc;
        if (int rc = A.add(&d->cov_work, cwork, 1)) return rc;
    }
    if (int rc = A.add(&d->tile_len, tlen)) return rc;
    if (int rc = A.add(&d->tile_contig_dev, tcont)) return rc;
    return MSNV_OK;
}

// host staging: every sample's intervals, filtered and made linear, and its (tile, sample) runs of them
void Finalize::coverage_runs_host(std::vector<Pair32> &iv, std::vector<uint64_t> &cvbase, std::vector<CP> &flat) {
    std::vector<std::vector<CP>> per(S);
    for (size_t s = 0; s < S; ++s) {
        const SampleCols &sc = ds.samples[s];
        uint32_t n_here = 0;
        for (size_t i = 0; i < sc.cov_tid.size(); ++i) {
            const size_t c = (size_t)sc.cov_tid[i];
            const int64_t L = ds.lengths[c];
            const int64_t b = sc.cov_beg[i];
            const bool minus_one = b > sc.cov_end[i];                          // {L, L - 1}: "-1 at L - 1" (pack_sample)
            const int64_t e = minus_one ? sc.cov_end[i] : (sc.cov_end[i] >= L ? L - 1 : sc.cov_end[i]);       // qaCompute.cpp:544-549
            if (!minus_one && b >= e) continue;
            const uint64_t g0 = (uint64_t)ds.tile_base[c] * TILE;
            const uint32_t idx = n_here++;
            iv.push_back(Pair32{(uint32_t)(g0 + (uint64_t)b), (uint32_t)(g0 + (uint64_t)e)});
            std::vector<CP> &pv = per[s];
            const uint32_t t_first = (uint32_t)((g0 + (uint64_t)(minus_one ? e : b)) / TILE), t_last = minus_one ? t_first : (uint32_t)((g0 + e - 1) / TILE);
            for (uint32_t t = t_first; t <= t_last; ++t) {
                size_t k = pv.size();
                while (k > 0 && pv[k - 1].tile > t) --k;
                if (k > 0 && pv[k - 1].tile == t) pv[k - 1].hi = idx + 1;
                else pv.insert(pv.begin() + (ptrdiff_t)k, CP{t, (uint32_t)s, idx, idx + 1});
            }
        }
        cvbase[s + 1] = cvbase[s] + n_here;
    }
    for (size_t s = 0; s < S; ++s) flat.insert(flat.end(), per[s].begin(), per[s].end());
}

// the pair tables by tile, the accumulator rows and the work items from the runs (the device's or the host's), wide items last
int Finalize::coverage_pairs_host(const std::vector<CP> &flat, const std::vector<uint64_t> &cvbase, std::vector<TilePair> &cpairs, std::vector<WorkItem> &cwork, bool in_thread) {
    // one pass for the tile counts, one for the pairs (sample order inside a tile comes with the order of `flat`) and the accumulator rows
    std::vector<uint32_t> cps(nt + 1, 0);
    for (const CP &p : flat) cps[p.tile + 1]++;
    for (uint64_t t = 0; t < nt; ++t) cps[t + 1] += cps[t];
    cpairs.resize(cps[nt]);
    {
        std::vector<uint32_t> fill(cps.begin(), cps.end() - 1);
        // blk_lo / nblk: absolute index of the sample's first interval (the kernel needs no per-sample base lookup)
        // max_depth: the accumulator row of the pair's (sample, contig) -- rows exist for the combinations that have intervals only
        ds.cov_row_sample.clear(); ds.cov_row_contig.clear(); ds.cov_row_start.assign(S + 1, 0);
        size_t i = 0;
        for (size_t s = 0; s < S; ++s) {
            ds.cov_row_start[s] = ds.cov_row_sample.size();
            uint32_t last_contig = UINT32_MAX;
            for (; i < flat.size() && flat[i].sample == s; ++i) {                     // (tile order = contig order)
                const CP &p = flat[i];
                const uint32_t c = ds.tile_contig[p.tile];
                if (c != last_contig) { ds.cov_row_sample.push_back((uint32_t)s); ds.cov_row_contig.push_back(c); last_contig = c; }
                if (ds.cov_row_sample.size() > 0xffffffffull) return fail(MSNV_EDOMAIN, "more than 2^32 (sample, contig) pairs with coverage in one shard");
                cpairs[fill[p.tile]++] = TilePair{p.sample, p.lo, p.hi, (uint32_t)(ds.cov_row_sample.size() - 1), (uint32_t)cvbase[s], (uint32_t)(cvbase[s] >> 32), 0, 0};
            }
        }
        ds.cov_row_start[S] = ds.cov_row_sample.size();
    }
    if (!in_thread) fin_trace("    cov tables: pairs by tile, rows");
    cwork.reserve(cpairs.size() / 2 + nt + 16);
    // a coverage work item = COV_ITEM_PAIRS consecutive pairs of a tile = one wavefront of msnv_coverage_tiles, which loads their
    // descriptors up front and a pair's intervals while it works on the pair before (fewer when one pair alone is deep:
    // MSNV_COV_ITEM intervals)
    const uint64_t cov_item_intervals = knob::cov_item_intervals();
    for (uint64_t t = 0; t < nt; ++t) {
        uint32_t lo = cps[t]; uint64_t acc = 0;
        for (uint32_t k = cps[t]; k < cps[t + 1]; ++k) {
            acc += cpairs[k].read_hi - cpairs[k].read_lo;
            if (acc >= cov_item_intervals || k + 1 - lo >= COV_ITEM_PAIRS || k + 1 == cps[t + 1]) { cwork.push_back(WorkItem{(uint32_t)t, lo, k + 1, 0, 0, 0, 0, 0, ChunkDesc{}}); lo = k + 1; acc = 0; }
        }
    }
    // the items with a pair of more than 32 767 intervals go last: msnv_coverage_tiles<true> (one word per position) runs them,
    // the 16-bit difference array of the usual variant holds +-32 767 per position and per 16 positions of one parity
    // (MSNV_COV_NARROW_MAX is read per dataset: tests lower it to run the other variant)
    const uint32_t cov_narrow_max = knob::cov_narrow_max();
    auto cov_wide = [&](const WorkItem &w) { for (uint32_t k = w.pair_lo; k < w.pair_hi; ++k) if (cpairs[k].read_hi - cpairs[k].read_lo > cov_narrow_max) return true; return false; };
    bool any_wide = false;
    for (const TilePair &q : cpairs) if (q.read_hi - q.read_lo > cov_narrow_max) { any_wide = true; break; }
    d->n_cov_work_wide = 0;
    if (any_wide) {
        const auto first_wide = std::stable_partition(cwork.begin(), cwork.end(), [&](const WorkItem &w) { return !cov_wide(w); });
        d->n_cov_work_wide = (uint32_t)(cwork.end() - first_wide);
    }
    if (!in_thread) fin_trace("    cov tables: work items");
    d->n_cov_pairs = (uint32_t)cpairs.size(); d->n_cov_work = (uint32_t)cwork.size();
    return MSNV_OK;
}

// ---- reference: nt16 codes (N beyond the contig end, as mpileup prints) + lower-case bits
int Finalize::reference() {
    ref4.assign(npos / 8 + 1, 0xffffffffu);
    std::vector<uint32_t> lc(npos / 32 + 1, 0u);
    // (contigs start on tile boundaries: their words of both tables are disjoint, so the contigs are dealt to the host threads --
    // a database shard is gigabases of FASTA)
    std::vector<size_t> with_seq;
    for (size_t c = 0; c < NC; ++c) if (ds.sel[c] && ds.has_seq[c]) with_seq.push_back(c);
    // the device pack has converted the selected contigs once already (devpack.hip: build_tables -- codes 8 per word, lower-case bits 32 per
    // word, per contig): a contig starts on a tile, so its words go into place as they are
    const bool converted = ds.dp.ready && !ds.dp.h_codes.empty();
    std::vector<size_t> by_char;
    for (size_t c : with_seq) {
        const uint64_t n = std::min<uint64_t>(ds.seqs[c].size(), (uint64_t)maxend[c]);
        if (!converted || n != ds.seqs[c].size() || ds.dp.h_code_off[c] == ~0ull) { by_char.push_back(c); continue; }      // (a FASTA record longer than its contig's tiles: character by character)
        const uint64_t g0 = (uint64_t)ds.tile_base[c] * TILE;
        memcpy(ref4.data() + g0 / 8, ds.dp.h_codes.data() + ds.dp.h_code_off[c], ((n + 7) / 8) * 4);
        memcpy(lc.data() + g0 / 32, ds.dp.h_lc.data() + ds.dp.h_lc_off[c], ((n + 31) / 32) * 4);
    }
    parallel_for(by_char.size(), [&](size_t k) {
        const size_t c = by_char[k];
        const std::string &s = ds.seqs[c];
        const uint64_t g0 = (uint64_t)ds.tile_base[c] * TILE;
        const uint64_t lim = std::min<uint64_t>(s.size(), (uint64_t)maxend[c]);
        for (uint64_t i = 0; i < lim; ++i) {
            const uint64_t g = g0 + i;
            const uint32_t code = nt16_of_char((unsigned char)s[i]);
            ref4[g >> 3] = (ref4[g >> 3] & ~(0xfu << (4 * (g & 7)))) | code << (4 * (g & 7));
            const char ch = s[i];
            if (ch == 'a' || ch == 'c' || ch == 'g' || ch == 't') lc[g >> 5] |= 1u << (g & 31);
        }
    });
    if (int rc = arena.add(&d->ref4, ref4)) return rc;
    if (int rc = arena.add(&d->ref_lc, lc)) return rc;
    ds.info.bytes_ref = npos / 2;
    fin_trace("reference");
    return MSNV_OK;
}

// ---- callable range per tile (BED -l regions; without BED every covered position)
int Finalize::callable_ranges() {
    vb_host.assign(nt + 1, 0); ve_host.assign(nt + 1, 0);
    for (uint64_t t = 0; t < nt; ++t) {
        const size_t c = ds.tile_contig[t];
        const int64_t t0 = (int64_t)(t - ds.tile_base[c]) * TILE;
        int64_t b = ds.has_bed ? ds.bed_beg[c] : 0, e = ds.has_bed ? ds.bed_end[c] : INT64_MAX;
        b = std::min<int64_t>(std::max<int64_t>(b - t0, 0), TILE);
        e = std::min<int64_t>(std::max<int64_t>(e - t0, 0), TILE);
        vb_host[t] = (uint32_t)b; ve_host[t] = (uint32_t)e;
    }
    if (int rc = arena.add(&d->tile_vbeg, vb_host)) return rc;
    if (int rc = arena.add(&d->tile_vend, ve_host)) return rc;

    fin_trace("callable ranges");
    return MSNV_OK;
}

// ---- per sample: gpos, tile overlap index; concatenate columns
int Finalize::layout_samples() {
    if (!R.fast) {
        std::atomic<int> split_err{0}; std::mutex split_mu; std::string split_msg;
        parallel_for(S, [&](size_t s) {
            if (int rc = split_deep_runs(ds.samples[s], device)) { std::lock_guard<std::mutex> lk(split_mu); if (!split_err.load()) { split_msg = msnv_last_error(); split_err.store(rc); } }
        });
        if (split_err.load()) return fail(split_err.load(), "%s", split_msg.c_str());
    }
    uint64_t all_pieces = 0, all_bases = 0;
    for (const SampleCols &sc : ds.samples) { all_pieces += R.fast ? (size_t)sc.n_dev_pieces : sc.hdr.size(); all_bases += sc.n_pileup_bases; }
    R.dense = layout_dense(all_pieces, all_bases);
    d->dense = R.dense;
    if (R.dense && R.fast) {
        if (int rc = devfin_dense(ds)) return rc;                    // devfin.hip: block streams, descriptors and run tables of every sample, in HBM
    } else if (R.dense) {
        for (size_t s = 0; s < S; ++s) if (ds.samples[s].on_device) { if (int rc = dev_set_device(device)) return rc; if (int rc = devpack_sample_to_host(ds.samples[s])) return rc; }
        parallel_for(S, [&](size_t s) {
            SampleCols &sc = ds.samples[s];
            relayout_dense(sc);
            for (int i = 0; i < 32; ++i) sc.seq.push_back(0xff);     // tail padding as in pack_sample
            while (sc.qual.size() < 2 * sc.seq.size()) sc.qual.push_back(0);
        });
    }
    rbase.assign(S + 1, 0); sbase.assign(S + 1, 0); bbase.assign(S + 1, 0);
    for (size_t s = 0; s < S; ++s) {
        bbase[s + 1] = bbase[s] + (R.fast ? (size_t)ds.samples[s].n_dev_blk : ds.samples[s].blk.size());
        rbase[s + 1] = rbase[s] + (R.fast ? (size_t)ds.samples[s].n_dev_pieces : ds.samples[s].hdr.size());
        const size_t seq_bytes = ds.samples[s].on_device ? (size_t)ds.samples[s].d_seq_bytes : ds.samples[s].seq.size();
        sbase[s + 1] = sbase[s] + ((seq_bytes + 15) & ~(size_t)15);
    }
    return MSNV_OK;
}

int Finalize::pairs_per_sample() {
    per_sample.assign(S, {});
    ds.first_tid = -1; ds.first_pos = -1;
    if (R.fast) for (size_t s = 0; s < S; ++s) {                           // the runs of pieces as the device found them (devpack.hip: msnv_pair_starts / msnv_pair_maxd)
        const SampleCols &sc = ds.samples[s];
        std::vector<PairTmp> &pv = per_sample[s];
        pv.reserve(sc.dev_pairs.size());
        for (const DevPair &p : sc.dev_pairs)
            pv.push_back(PairTmp{ds.tile_base[(size_t)p.tid] + p.tile, (uint32_t)s, p.lo, p.hi, p.maxd, (uint32_t)pv.size(), p.grp});
    }
    else parallel_for(S, [&](size_t s) {
        SampleCols &sc = ds.samples[s];
        std::vector<PairTmp> &pv = per_sample[s];
        // pieces are grouped by tile: one pair per run
        for (size_t i = 0; i < sc.hdr.size(); ++i) {
            const size_t c = (size_t)sc.tid[i];
            const uint64_t gs = (uint64_t)ds.tile_base[c] * TILE + sc.hdr[i].gpos;
            sc.hdr[i].gpos = (uint32_t)gs;
            const uint32_t t = (uint32_t)(gs / TILE);
            if (!R.dense && !sc.on_device) {                       // (device-packed samples: devfin.hip msnv_fill_padding, once the columns are in place)
                // The alignment padding behind a piece (up to the next 16 bases) reads as the reference the kernel compares
                // it with (N beyond the tile): msnv_pileup_tiles_narrow32 then masks mismatch flags per 16 bases, not per base.
                const uint32_t len = sc.hdr[i].cig, stop = (len + 2u * SEQ_ALIGN - 1u) & ~(2u * SEQ_ALIGN - 1u);
                uint8_t *sp = sc.seq.data() + sc.hdr[i].seqoff;
                for (uint32_t j = len; j < stop; ++j) {
                    const uint64_t g = gs + j;
                    const uint32_t code = (gs % TILE + j < TILE) ? (ref4[g >> 3] >> (4 * (g & 7))) & 0xfu : 0xfu;
                    const int sh = (int)(j & 1u) * 4;
                    sp[j >> 1] = (uint8_t)((sp[j >> 1] & ~(0xf << sh)) | code << sh);
                }
            }
            if (!pv.empty() && pv.back().tile == t && pv.back().grp == sc.grp[i]) pv.back().hi = (uint32_t)i + 1;
            else pv.push_back(PairTmp{t, (uint32_t)s, (uint32_t)i, (uint32_t)i + 1, 0, (uint32_t)pv.size(), sc.grp[i]});
        }
        for (PairTmp &p : pv) {       // depth bound: every read alive inside the tile was alive when one of [lo,hi) started
            uint32_t m = 0;
            for (uint32_t i = p.lo; i < p.hi; ++i) m = std::max<uint32_t>(m, sc.depth[i]);
            p.maxd = m;
        }
    });
    for (size_t s = 0; s < S; ++s) {
        const SampleCols &sc = ds.samples[s];
        tot_reads += R.fast ? (size_t)sc.n_dev_pieces : sc.hdr.size(); tot_pile_reads += sc.n_pileup_reads; tot_bases += sc.n_pileup_bases;
        if (sc.first_tid >= 0 && (ds.first_tid < 0 || sc.first_tid < ds.first_tid || (sc.first_tid == ds.first_tid && sc.first_beg < ds.first_pos))) {
            ds.first_tid = sc.first_tid; ds.first_pos = sc.first_beg;
        }
    }
    fin_trace("pairs per sample");
    return MSNV_OK;
}

// ---- CSR of pairs by tile (sample order inside a tile)
int Finalize::pair_csr() {
    tps.assign(nt + 1, 0);
    for (size_t s = 0; s < S; ++s) for (const PairTmp &p : per_sample[s]) tps[p.tile + 1]++;
    for (uint64_t t = 0; t < nt; ++t) tps[t + 1] += tps[t];
    pairs.assign(tps[nt], TilePair{});
    std::vector<uint32_t> fill(tps.begin(), tps.end() - 1);
    for (size_t s = 0; s < S; ++s)
        for (const PairTmp &p : per_sample[s]) {
            const SampleCols &sc = ds.samples[s];
            TilePair tp{p.sample, p.lo, p.hi, p.maxd, 0, 0, 0, p.grp ? 1u : 0u};      // pad = 1: one of several pairs of this sample in the tile
            if (R.dense) {
                if (p.run >= sc.run_nblk.size()) return fail(MSNV_EINVAL, "internal: dense runs and tile pairs disagree");
                tp.blk_lo = sc.run_blk_lo[p.run]; tp.nblk = sc.run_nblk[p.run]; tp.seq0 = sc.run_seq0[p.run];
            }
            pairs[fill[p.tile]++] = tp;
        }
    return MSNV_OK;
}

int Finalize::pair_classes() {
    fuse_tile.assign(nt, 0);
    // inside a tile: narrow pairs (every per-position count fits a byte) first, then wide ones, then the SHALLOW pairs that
    // are merged into groups (msnv_pileup_tiles_merged): pad = 2.  A pair of ~20 pieces costs the narrow kernel a chunk
    // iteration and a pass over all 2048 positions whatever it holds, so cohorts of many shallow samples (1600 x 1x ran at
    // 24 % of the roofline) and contigs much shorter than a tile put several pairs into the same bins.
    // MSNV_SHALLOW_PIECES: number of pieces up to which a pair counts as shallow (default 48 = 3/8 of a chunk; 0 = never
    // merge); its depth bound must leave room for at least three pairs in a group, and a tile needs two such pairs.
    const uint32_t shallow_pieces = knob::shallow_pieces();   // read per dataset (tests switch it)
    const bool can_merge = !R.dense && shallow_pieces > 0 && sbase[S] < ((uint64_t)SEQ_ALIGN << 37);   // merged headers hold absolute seq offsets / SEQ_ALIGN in 37 bits
    auto is_shallow = [&](const TilePair &p) { return p.read_hi - p.read_lo <= shallow_pieces && p.max_depth <= MERGE_MAX_DEPTH / 3 && !p.pad; };
    // ... and only when the shallow pairs are a real share of the dataset (>= 3 % of its pieces): a few of them -- the
    // partial last tile of every contig of the benchmark shape -- are not worth the second code path in the tail
    std::vector<uint8_t> merge_tile(nt, 0);
    // Whole-tile work items: in a SPARSE cohort (a pair or two per tile: BASELINE configs[3]) a tile whose pairs fit ONE merged group
    // is piled up by one workgroup, which then holds the tile's totals and applies the gates itself (kernels.hip: fused_tile_gate).
    // MSNV_FUSE=0 switches it off, MSNV_FUSE_PIECES sets the pieces a pair may hold (default 256), MSNV_FUSE=1 forces it on
    // whatever the cohort looks like (tests).
    {
        uint64_t tiles_with_pairs = 0;
        for (uint64_t t = 0; t < nt; ++t) tiles_with_pairs += tps[t + 1] > tps[t];
        const char forced = knob::fuse();
        const bool sparse = tiles_with_pairs && pairs.size() < 4 * tiles_with_pairs;
        const bool fuse_on = can_merge && forced != '0' && (sparse || forced == '1');
        const uint32_t fuse_pieces = knob::fuse_pieces();
        if (fuse_on) for (uint64_t t = 0; t < nt; ++t) {
            const uint32_t n = tps[t + 1] - tps[t];
            if (n == 0 || n > MERGE_MAX_PAIRS) continue;
            uint64_t depth = 0; bool ok = true;
            for (uint32_t k = tps[t]; k < tps[t + 1] && ok; ++k) { depth += pairs[k].max_depth; ok = !pairs[k].pad && pairs[k].read_hi - pairs[k].read_lo <= fuse_pieces; }
            if (ok && depth <= MERGE_MAX_DEPTH) fuse_tile[t] = 1;
        }
    }
    if (can_merge) {
        uint64_t shallow_pieces_total = 0, all_pieces = 0;
        for (uint64_t t = 0; t < nt; ++t) {
            uint32_t n_shallow = 0; uint64_t np = 0;
            for (uint32_t k = tps[t]; k < tps[t + 1]; ++k) { all_pieces += pairs[k].read_hi - pairs[k].read_lo; if (is_shallow(pairs[k])) { ++n_shallow; np += pairs[k].read_hi - pairs[k].read_lo; } }
            if (n_shallow >= 2) { merge_tile[t] = 1; shallow_pieces_total += np; }
        }
        const bool force = knob::merge_always();   // (tests)
        if (!force && shallow_pieces_total * 100 < all_pieces * 3) std::fill(merge_tile.begin(), merge_tile.end(), 0);
    }
    for (uint64_t t = 0; t < nt; ++t) {
        auto b = pairs.begin() + tps[t], e = pairs.begin() + tps[t + 1];
        if (fuse_tile[t]) for (auto it = b; it != e; ++it) it->pad = 2;
        else if (merge_tile[t]) for (auto it = b; it != e; ++it) if (is_shallow(*it)) it->pad = 2;
        auto cls = [](const TilePair &p) { return p.pad == 2 ? 2 : p.max_depth < NARROW_MAX_DEPTH ? 0 : 1; };
        bool in_class_order = true;                              // (nearly every tile's pairs are of one class: the sort's temporary buffer per tile was a third of this stage)
        for (auto it = b; it != e && it + 1 != e; ++it) if (cls(*(it + 1)) < cls(*it)) { in_class_order = false; break; }
        if (!in_class_order) std::stable_sort(b, e, [&](const TilePair &x, const TilePair &y) { return cls(x) < cls(y); });
    }
    tpm.assign(nt + 1, 0);
    for (uint64_t t = 0; t < nt; ++t) { uint32_t k = tps[t]; while (k < tps[t + 1] && pairs[k].pad != 2) ++k; tpm[t] = k; }
    fin_trace("pair CSR, merge / fuse classes");
    return MSNV_OK;
}

// ---- slots: the samples that have reads in a tile are numbered 0 .. n - 1 (the pairs of a split sample, consecutive, share
// one); the per-sample cells of the tile's called positions are stored per slot (kernels.hip: CellMap) and the host expands
// to all samples when it fetches.  From here on TilePair::pad = kind (0 narrow or wide, 1 split, 2 merged) | slot << 8.
int Finalize::slots() {
    ds.tile_slot_base.assign(nt + 1, 0);
    ds.slot_sample.clear();
    std::vector<uint32_t> nslots(nt + 1, 0);
    for (uint64_t t = 0; t < nt; ++t) {
        ds.tile_slot_base[t] = (uint64_t)ds.slot_sample.size();
        uint32_t n = 0;
        for (uint32_t k = tps[t]; k < tps[t + 1]; ++k) {
            const bool same = k > tps[t] && pairs[k].pad == 1 && (pairs[k - 1].pad & 0xffu) == 1 && pairs[k].sample == pairs[k - 1].sample;
            if (!same) { ds.slot_sample.push_back(pairs[k].sample); ++n; }
            pairs[k].pad |= (n - 1u) << 8;
        }
        // the device's row stride: tiles of >= 16 slots get rows that are multiples of 16 bytes (8 coverage cells), so that the
        // many-site gather can write them with 16-byte stores (kernels.hip: gather_cov_wide); the padding cells stay zero
        nslots[t] = n >= 16u ? (n + 7u) & ~7u : n;
    }
    ds.tile_slot_stride = nslots;
    ds.tile_slot_base[nt] = (uint64_t)ds.slot_sample.size();
    // the device's copy also says whether some sample of the tile was split into several pairs (device.h: NSLOTS_SPLIT): several
    // allele events may then meet in one cell and are added; in every other tile a cell has one writer (kernels.hip: scatter_events_block)
    for (uint64_t t = 0; t < nt; ++t)
        for (uint32_t k = tps[t]; k < tps[t + 1]; ++k) if ((pairs[k].pad & 0xffu) == 1u) { nslots[t] |= NSLOTS_SPLIT; break; }
    if (int rc = arena.add(&d->tile_nslots, nslots)) return rc;
    fin_trace("slots");
    return MSNV_OK;
}

// ---- work list: split each tile's pairs so that work items carry similar read counts
int Finalize::work_list() {
    uint64_t total_reads_in_pairs = 0;
    for (const TilePair &p : pairs) total_reads_in_pairs += p.read_hi - p.read_lo;
    // work item size: pieces per workgroup.  MSNV_ITEM_PIECES overrides (tuning experiments).
    // ~1000 pieces (a few (tile, sample) pairs) per workgroup: measured on the benchmark shape (16 M pieces, one box,
    // pileup kernel): 400 -> 0.616 ms, 700 -> 0.614, 1000 -> 0.599-0.615, 1500 -> 0.608-0.633, 2628 -> 0.636-0.644.
    // Small items keep the last wave of workgroups short (an item of 2600 pieces runs ~190 us of a 640 us kernel);
    // below ~700 the per-item costs (LDS init, partial row, gate summing more rows) take over.
    // (at 4x the benchmark size 1000 still beats 2000: 55.5 vs 54.5 % of the roofline, so the size is a constant)
    // Items stay in tile order: dispatching the longest items first (shorter last wave of workgroups) measured 3 % SLOWER
    // (0.595 -> 0.612 ms) -- neighbouring items of a tile share the reference and the allele-total lines in L2.
    // (round 3, after the kernel had lost 9 % of its time: 1000 -> 0.5544 ms kernel / 0.6269 ms pass, 1400 -> 0.5520 / 0.6232,
    // 2000 -> 0.5510 / 0.6197, 2800 -> 0.5536 / 0.6235 over four alternations, profiles/r03k_ab_items.txt: flat in the kernel, the gate
    // kernel sums fewer partial rows)
    uint64_t target = knob::item_pieces();
    std::vector<WorkItem> wide, merged;
    auto chunks_of = [&](const TilePair &q) -> uint64_t {
        const bool nar = q.max_depth < NARROW_MAX_DEPTH;
        if (R.dense && nar) return (q.nblk + DENSE_CHUNK_BLOCKS - 1) / DENSE_CHUNK_BLOCKS;
        return (q.read_hi - q.read_lo + CHUNK_READS - 1) / CHUNK_READS;
    };
    // Taper: the items of the last tiles are cut smaller, so that the last wave of workgroups (dispatch is in index order)
    // ends on short items.  The thresholds are in units of one full wave of workgroups (resident workgroups x pieces per
    // item), not fractions of the dataset: on the benchmark shape (16 M pieces) they are the last 20 / 8 / 3 %, at
    // BASELINE configs[2] scale (514 M pieces) the last 0.6 % -- tapering a fixed fraction there cost 5 %.
    // MSNV_ITEM_TAPER=0 switches it off; MSNV_TAPER_AT=u1,u2,u3 moves the thresholds.
    const bool taper = knob::item_taper();   // read per dataset (tests switch it)
    const knob::TaperAt at = knob::taper_at();
    const double u1 = at.u1, u2 = at.u2, u3 = at.u3;
    const uint64_t base_target = target;
    const double wave_pieces = (double)dev_resident_workgroups(7) * (double)base_target;   // 7 workgroups of 256 threads per CU (kernels.hip)
    uint64_t seen = 0;
    for (uint64_t t = 0; t < nt; ++t) {
        uint32_t lo = tps[t];
        uint64_t acc = 0, nch = 0;
        if (taper && total_reads_in_pairs) {
            const double left = (double)(total_reads_in_pairs - seen) / wave_pieces;
            target = left < u3 ? std::max<uint64_t>(64, base_target / 8) : left < u2 ? std::max<uint64_t>(64, base_target / 4) : left < u1 ? std::max<uint64_t>(64, base_target / 2) : base_target;
        }
        // merged groups: consecutive shallow pairs whose depth bounds add up to <= MERGE_MAX_DEPTH; an item = whole groups
        {
            uint32_t g_lo = tpm[t], i_lo = tpm[t];
            uint64_t g_depth = 0, i_pieces = 0, i_chunks = 0, g_pieces = 0;
            for (uint32_t k = tpm[t]; k < tps[t + 1]; ++k) {
                const uint32_t nr = pairs[k].read_hi - pairs[k].read_lo;
                seen += nr;
                if (k > g_lo && (g_depth + pairs[k].max_depth > MERGE_MAX_DEPTH || k - g_lo >= MERGE_MAX_PAIRS)) {   // close the group
                    groups.push_back(MergedGroup{g_lo, k, (uint32_t)t});
                    i_pieces += g_pieces; i_chunks += (g_pieces + CHUNK_READS - 1) / CHUNK_READS;
                    g_lo = k; g_depth = 0; g_pieces = 0;
                    if (i_pieces >= target || i_chunks >= MAX_CHUNKS_PER_ITEM / 2) { merged.push_back(WorkItem{(uint32_t)t, i_lo, k, 0, 0, 0, 0, 0, ChunkDesc{}}); i_lo = k; i_pieces = 0; i_chunks = 0; }
                }
                g_depth += pairs[k].max_depth; g_pieces += nr;
            }
            if (tps[t + 1] > g_lo) { groups.push_back(MergedGroup{g_lo, tps[t + 1], (uint32_t)t}); merged.push_back(WorkItem{(uint32_t)t, i_lo, tps[t + 1], 0, 0, 0, 0, 0, ChunkDesc{}}); }
        }
        for (uint32_t k = tps[t]; k < tpm[t]; ++k) {
            const uint32_t nr = pairs[k].read_hi - pairs[k].read_lo;
            seen += nr;
            acc += nr; nch += chunks_of(pairs[k]);
            const bool narrow = pairs[k].max_depth < NARROW_MAX_DEPTH;
            const bool boundary = k + 1 == tpm[t] || (narrow != (pairs[k + 1].max_depth < NARROW_MAX_DEPTH));
            const uint64_t next_ch = boundary ? 0 : chunks_of(pairs[k + 1]);
            if (acc >= target || boundary || nch + next_ch > MAX_CHUNKS_PER_ITEM) {
                (narrow ? work : wide).push_back(WorkItem{(uint32_t)t, lo, k + 1, 0, 0, 0, 0, 0, ChunkDesc{}}); lo = k + 1; acc = 0; nch = 0;
            }
        }
    }
    // whole-tile items behind the other merged items: the pileup kernel picks its code by the range a work item is in
    // (and among them the tiles with ONE pair last: their per-sample cells are the tile's totals, written by the gate kernel -- the
    // merged gather skips their groups, the last n_groups_solo of its list)
    for (uint64_t t = 0; t < nt; ++t) if (fuse_tile[t] && tps[t + 1] - tps[t] == 1) fuse_tile[t] = 2;
    std::stable_sort(merged.begin(), merged.end(), [&](const WorkItem &x, const WorkItem &y) { return fuse_tile[x.tile] < fuse_tile[y.tile]; });
    std::stable_sort(groups.begin(), groups.end(), [&](const MergedGroup &x, const MergedGroup &y) { return fuse_tile[x.tile] < fuse_tile[y.tile]; });
    d->n_groups_solo = 0;
    for (const MergedGroup &g : groups) d->n_groups_solo += fuse_tile[g.tile] == 2;
    d->n_work_narrow = (uint32_t)work.size();
    d->n_work_merged = (uint32_t)merged.size();
    d->n_work_fused = 0;
    for (const WorkItem &w : merged) d->n_work_fused += fuse_tile[w.tile] != 0;
    work.insert(work.end(), merged.begin(), merged.end());
    work.insert(work.end(), wide.begin(), wide.end());
    fin_trace("work list");
    return MSNV_OK;
}

// ---- coverage partials: one row of TILE counters per work item, rows of a tile contiguous (the gate kernel sums them):
// u8 rows first (narrow items whose pairs' depth bounds add up to < 256: most of them at ~10x), then u16 rows (the other
// narrow items: <= 32 pairs x 254), then the u32 rows of wide items.  Bit 0 of part_lo marks a u8 row, bits 1-2 hold the tile's allele-total mode.
int Finalize::partial_rows() {
    std::vector<uint32_t> tss(nt + 1, 0), t16(nt + 1, 0), twide(nt + 1, 0);
    for (const WorkItem &w : work) ++tss[w.tile + 1];
    for (uint64_t t = 0; t < nt; ++t) tss[t + 1] += tss[t];
    std::vector<uint8_t> cls(work.size(), 0);
    // Allele totals (kernels.hip: tot_add / msnv_gate_sites): a tile's 4 x TILE words hold its mismatch totals position by
    // position, as narrow as the tile's summed depth bound allows -- 4 bytes (A, C, G, T) in ONE word per position when the
    // bound is below 256 (a sparse cohort: the gate kernel then reads 4 B per position instead of 16), 2 x u16 in two words
    // below 65536 (the benchmark shape), else four words.  MSNV_TOT_MODE=0..2 sets the narrowest mode allowed (tests).
    std::vector<uint64_t> tile_bound(nt, 0);
    for (size_t i = 0; i < work.size(); ++i) {
        uint64_t bound = 0;
        for (uint32_t k = work[i].pair_lo; k < work[i].pair_hi; ++k) bound += pairs[k].max_depth;
        tile_bound[work[i].tile] += bound;
        cls[i] = i >= d->n_work_narrow + d->n_work_merged ? 2 : bound < 256 ? 0 : 1;
    }
    const uint32_t min_tot_mode = knob::tot_mode_min();
    auto tot_mode = [&](uint64_t t) { return std::max<uint32_t>(min_tot_mode, tile_bound[t] < 256 ? 0u : tile_bound[t] < 65536 ? 1u : 2u); };
    std::vector<uint32_t> fill(tss.begin(), tss.end() - 1);
    std::vector<uint8_t> slot_cls(work.size(), 0);
    for (int c = 0; c < 3; ++c)
        for (size_t i = 0; i < work.size(); ++i)
            if (cls[i] == c) { work[i].slot = fill[work[i].tile]++; slot_cls[work[i].slot] = (uint8_t)c; }
    std::vector<uint64_t> off(work.size() + 1, 0);
    for (size_t s = 0; s < work.size(); ++s) off[s + 1] = off[s] + ((uint64_t)TILE << slot_cls[s]);
    for (size_t i = 0; i < work.size(); ++i) {
        WorkItem &w = work[i];
        w.part_lo = (uint32_t)off[w.slot] | (cls[i] == 0 ? 1u : 0u) | tot_mode(w.tile) << 1 | (fuse_tile[w.tile] ? WORK_FUSED : 0u); w.part_hi = (uint32_t)(off[w.slot] >> 32);
    }
    for (uint64_t t = 0; t < nt; ++t) {                    // first u16 row and first u32 row of every tile
        uint32_t s = tss[t];
        while (s < tss[t + 1] && slot_cls[s] < 1) ++s;
        t16[t] = s;
        while (s < tss[t + 1] && slot_cls[s] < 2) ++s;
        twide[t] = s;
    }
    std::vector<uint32_t> active;
    for (uint64_t t = 0; t < nt; ++t) if (tss[t + 1] > tss[t]) active.push_back((uint32_t)t);
    d->n_active_tiles = (uint32_t)active.size();
    if (int rc = arena.add(&d->active_tiles, active, 1)) return rc;
    // the spill gather only has something to do in tiles that hold pairs outside merged groups (the others -- every tile of a sparse
    // cohort -- would each cost a workgroup that looks its tile up and leaves)
    {
        std::vector<uint32_t> gather_tiles;
        for (uint32_t t : active) if (tpm[t] > tps[t]) gather_tiles.push_back(t);
        d->n_gather_tiles = (uint32_t)gather_tiles.size();
        if (int rc = arena.add(&d->gather_tiles, gather_tiles, 1)) return rc;
    }
    d->part_bytes = std::max<uint64_t>(16, off[work.size()]);
    if (int rc = arena.add(&d->tile_slot_start, tss)) return rc;
    if (int rc = arena.add(&d->tile_slot_u16, t16)) return rc;
    if (int rc = arena.add(&d->tile_slot_wide, twide)) return rc;
    if (int rc = arena.add(&d->slot_off, off)) return rc;
    // one descriptor per active tile for the gate kernel: everything it looks up about its tile in one load
    std::vector<uint32_t> nslots_host(nt + 1, 0);
    for (uint64_t t = 0; t < nt; ++t) nslots_host[t] = ds.tile_slot_stride[t];
    std::vector<GateTile> gts;
    gts.reserve(active.size());
    for (uint32_t t : active) gts.push_back(GateTile{t, tss[t], t16[t], twide[t], tss[t + 1], vb_host[t], ve_host[t], nslots_host[t], off[tss[t]], tot_mode(t), (uint32_t)fuse_tile[t],
                                                                  tps[t], tpm[t] - tps[t], 0, 0});
    if (int rc = arena.add(&d->gate_tiles, gts, 1)) return rc;
    d->gather_split = knob::gather_split((uint32_t)std::min<uint64_t>(4, std::max<uint64_t>(1, (active.empty() ? 0 : pairs.size() / active.size()) / 32)));
    {   // whole-tile work items write their candidate records per active tile
        std::vector<uint32_t> stage_idx(nt + 1, 0xffffffffu);
        uint32_t n_fused = 0;
        for (size_t i = 0; i < active.size(); ++i) { stage_idx[active[i]] = (uint32_t)i; n_fused += fuse_tile[active[i]] != 0; }
        d->n_fused_tiles = n_fused;
        if (n_fused) {
            std::vector<GateTile> dense_l, staged_l;
            for (size_t i = 0; i < gts.size(); ++i) {
                if (!gts[i].staged) { dense_l.push_back(gts[i]); continue; }
                GateTile g = gts[i];
                g.row0 = (uint64_t)i;                              // (a whole-tile item writes no partial row: the field carries the index of its record list)
                staged_l.push_back(g);
            }
            if (int rc = arena.add(&d->gate_tiles_dense, dense_l, 1)) return rc;
            if (int rc = arena.add(&d->gate_tiles_staged, staged_l, 1)) return rc;
            if (int rc = arena.add(&d->tile_stage_idx, stage_idx)) return rc;
        }
    }
    d->wide_tot = false;
    for (uint32_t t : active) if (tot_mode(t) == 2u) d->wide_tot = true;
    d->use_dirty = !active.empty() && work.size() < 4 * active.size();       // a sparse cohort: fewer than four work items per tile
    fin_trace("partial rows, gate tiles");
    return MSNV_OK;
}

// ---- chunk descriptors of the merged groups: their piece headers, group by group, and chunks that run across the group's pairs
int Finalize::merged_chunks() {
    size_t gi = 0;
    for (uint32_t wi = d->n_work_narrow; wi < d->n_work_narrow + d->n_work_merged; ++wi) {
        WorkItem &w = work[wi];
        w.chunk_lo = (uint32_t)mchunks.size();
        for (; gi < groups.size() && groups[gi].pair_lo >= w.pair_lo && groups[gi].pair_hi <= w.pair_hi; ++gi) {
            const MergedGroup &g = groups[gi];
            const uint64_t h0 = R.fast ? hm_count : hm.size();
            for (uint32_t k = g.pair_lo; k < g.pair_hi; ++k) {
                const TilePair &p = pairs[k];
                if (R.fast) { hm_src.push_back(DevMergedSrc{k, k - g.pair_lo, hm_count}); hm_count += p.read_hi - p.read_lo; continue; }
                const SampleCols &sc = ds.samples[p.sample];
                for (uint32_t r = p.read_lo; r < p.read_hi; ++r) {
                    const uint64_t so = (sbase[p.sample] + sc.hdr[r].seqoff) >> SEQ_ALIGN_LOG2;          // 37 bits: bits 32-36 ride in bits 27-31 of the first word
                    hm.push_back(PieceHdr{(sc.hdr[r].gpos % TILE) | sc.hdr[r].cig << 11 | (k - g.pair_lo) << 19 | (uint32_t)(so >> 32) << 27, (uint32_t)so});
                }
            }
            const uint64_t n_h = (R.fast ? hm_count : hm.size()) - h0;
            mgroups.push_back(MergedGroupDev{h0, w.tile, g.pair_lo, g.pair_hi - g.pair_lo, (uint32_t)n_h});
            for (uint64_t r = 0; r < n_h; r += CHUNK_READS) {
                const uint32_t n = (uint32_t)std::min<uint64_t>(CHUNK_READS, n_h - r);
                mchunks.push_back(ChunkDesc{h0 + r, 0, pairs[g.pair_lo].sample, g.pair_lo, n | (r + n >= n_h ? 1u << 16 : 0u), g.pair_hi - g.pair_lo});
            }
        }
        w.chunk_hi = (uint32_t)mchunks.size();
    }
    if (gi != groups.size()) return fail(MSNV_EINVAL, "internal: merged groups and work items disagree");
    M = mchunks.size();
    if (M > 0x7ffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^31 chunks of merged groups in one shard");
    return MSNV_OK;
}

int Finalize::narrow_chunks() {
    hdr4_of.assign(HDR4 && !R.dense && !R.fast ? S : 0, {});
    for (size_t s = 0; s < hdr4_of.size(); ++s) hdr4_of[s].assign(ds.samples[s].hdr.size(), 0u);
    R.chunks_on_device = R.fast && !R.dense;
    if (R.chunks_on_device) {
        if (rbase[S] > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 pieces in one shard: shard the contigs further");      // (chunks <= pieces: the 32-bit scan of their counts cannot wrap)
        item_first.reserve((size_t)d->n_work_narrow + 1);
        for (uint32_t wi = 0; wi < d->n_work_narrow; ++wi) {
            item_first.push_back((uint32_t)narrow_pairs.size());
            for (uint32_t k = work[wi].pair_lo; k < work[wi].pair_hi; ++k) { narrow_pairs.push_back(k); chunk_cap += (pairs[k].read_hi - pairs[k].read_lo + CHUNK_READS - 1) / CHUNK_READS + 2; }
        }
        item_first.push_back((uint32_t)narrow_pairs.size());
        chunk_cap = knob::chunk_cap(chunk_cap);      // (tests: a table too small on purpose -> the exact, waiting form)
        if (M + chunk_cap > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 chunks in one shard");
    }
    else if (int rc = narrow_chunks_host()) return rc;
    fin_trace("chunks (host part)");
    if (!R.chunks_on_device) for (size_t wi = 0; wi < (size_t)d->n_work_narrow + d->n_work_merged; ++wi)
        if (work[wi].chunk_hi > work[wi].chunk_lo) work[wi].first = work[wi].chunk_lo < M ? mchunks[work[wi].chunk_lo] : nchunks[work[wi].chunk_lo - M];
    return MSNV_OK;
}

// the host's cut of every narrow work item's pairs into chunks
int Finalize::narrow_chunks_host() {
    for (uint32_t wi = 0; wi < d->n_work_narrow; ++wi) {
        WorkItem &w = work[wi];
        w.chunk_lo = (uint32_t)(M + nchunks.size());
        for (uint32_t k = w.pair_lo; k < w.pair_hi; ++k) {
            const TilePair &p = pairs[k];
            if (R.dense) {        // chunk = up to DENSE_CHUNK_BLOCKS blocks of the pair's stream: {first block, seq byte offset of that block}
                for (uint32_t b = 0; b < p.nblk; b += DENSE_CHUNK_BLOCKS) {
                    const uint32_t n = std::min<uint32_t>(DENSE_CHUNK_BLOCKS, p.nblk - b);
                    nchunks.push_back(ChunkDesc{bbase[p.sample] + p.blk_lo + b, sbase[p.sample] + p.seq0 + 16ull * b, p.pad >> 8, k,
                                                n | (b + n >= p.nblk ? 1u << 16 : 0u), p.pad & 0xffu});      // "sample" = the sample's slot in the tile
                }
                continue;
            }
            if (HDR4) {
                // a chunk = up to CHUNK_READS consecutive pieces whose seq bytes lie within 2^HDR4_OFF_BITS alignment units of the chunk's
                // lowest offset (always true for pieces in storage order; the pieces a read leaves in the NEXT tile sit a little before
                // that tile's other pieces); seq_base = the absolute offset of that lowest byte, the headers hold the distance to it
                const SampleCols &sc = ds.samples[p.sample];
                std::vector<uint32_t> &h4 = hdr4_of[p.sample];
                constexpr uint64_t span_max = (uint64_t)SEQ_ALIGN << HDR4_OFF_BITS;
                uint32_t r = p.read_lo;
                while (r < p.read_hi) {
                    uint64_t lo = sc.hdr[r].seqoff, hi = lo;
                    uint32_t e = r;
                    while (e < p.read_hi && e - r < CHUNK_READS) {
                        const uint64_t o = sc.hdr[e].seqoff, nlo = std::min(lo, o), nhi = std::max(hi, o);
                        if (nhi - nlo >= span_max) break;
                        lo = nlo; hi = nhi; ++e;
                    }
                    for (uint32_t i = r; i < e; ++i)
                        h4[i] = (sc.hdr[i].gpos % TILE) | sc.hdr[i].cig << 11 | (uint32_t)((sc.hdr[i].seqoff - lo) >> SEQ_ALIGN_LOG2) << 19;
                    nchunks.push_back(ChunkDesc{rbase[p.sample] + r, sbase[p.sample] + lo, p.pad >> 8, k, (e - r) | (e >= p.read_hi ? 1u << 16 : 0u), p.pad & 0xffu});
                    r = e;
                }
                continue;
            }
            for (uint32_t r = p.read_lo; r < p.read_hi; r += CHUNK_READS) {
                const uint32_t n = std::min<uint32_t>(CHUNK_READS, p.read_hi - r);
                nchunks.push_back(ChunkDesc{rbase[p.sample] + r, sbase[p.sample], p.pad >> 8, k, n | (r + n >= p.read_hi ? 1u << 16 : 0u), p.pad & 0xffu});
            }
        }
        w.chunk_hi = (uint32_t)(M + nchunks.size());
    }
    return MSNV_OK;
}

// ---- the index tables up, in one block; then the kernels that finish them are queued (nothing here waits for them)
int Finalize::upload_index() {
    d->n_pairs = (uint32_t)pairs.size(); d->n_work = (uint32_t)work.size();
    d->n_merged_groups = (uint32_t)mgroups.size();
    d->max_group_pairs = 0;
    for (const MergedGroupDev &g : mgroups) d->max_group_pairs = std::max(d->max_group_pairs, g.n_pairs);
    if (int rc = arena.add(&d->pairs, pairs)) return rc;
    if (int rc = arena.add(&d->s_read_base, rbase)) return rc;
    if (int rc = arena.add(&d->s_seq_base, sbase)) return rc;
    if (int rc = arena.add(&d->merged_groups, mgroups, 1)) return rc;
    if (int rc = arena.add(&d->tile_pair_merged, tpm)) return rc;
    if (int rc = arena.add(&d->tile_pair_start, tps)) return rc;
    if (int rc = arena.add(&d->work, work)) return rc;
    if (R.fast) {
        ds.info.bytes_headers += hm_count * sizeof(PieceHdr);
        d->n_hdr8m = hm_count;
    } else {
        ds.info.bytes_headers += hm.size() * sizeof(PieceHdr);
        d->n_hdr8m = hm.size();
        if (int rc = arena.add(&d->hdr8m, hm, 1)) return rc;
    }
    if (int rc = arena.commit(*d)) return rc;
    chunk_room = M + (R.chunks_on_device ? chunk_cap : nchunks.size());
    d->n_chunks = M + nchunks.size();                               // (fast, piece layout: the narrow chunks are counted behind finalize's last wait)
    if (int rc = dev_alloc((void **)&d->chunks, (chunk_room + 1) * sizeof(ChunkDesc), &d->device_bytes)) return rc;
    if (int rc = dev_upload(d->chunks, mchunks.data(), M * sizeof(ChunkDesc))) return rc;
    if (int rc = dev_upload(d->chunks + M, nchunks.data(), nchunks.size() * sizeof(ChunkDesc))) return rc;
    fin_trace("  index tables up");
    if (R.fast) {
        if (int rc = dev_alloc((void **)&d->hdr, (rbase[S] + 1) * sizeof(ReadHdr), &d->device_bytes)) return rc;
        if (int rc = dev_alloc((void **)&d->hdr8m, (hm_count + 1) * sizeof(PieceHdr), &d->device_bytes)) return rc;
    }
    if (R.chunks_on_device) {
        // the pieces are in HBM: the chunks of every narrow pair are cut there by a kernel that runs the same greedy rule as the loop above,
        // the work items learn their ranges there too
        if (int rc = dev_alloc((void **)&d->hdr4, (rbase[S] + 4) * sizeof(uint32_t), &d->device_bytes)) return rc;
        if (int rc = dev_memset_async(d->hdr4, 0, (rbase[S] + 4) * sizeof(uint32_t), stream)) return rc;
        if (int rc = devfin_chunks_launch(ds, *d, narrow_pairs, item_first, (uint32_t)M, chunk_cap)) return rc;
    }
    if (R.fast) {
        if (int rc = devfin_merged_headers(ds, *d, hm_src)) return rc;
        if (int rc = devfin_work_first(ds, *d, d->n_work_narrow + d->n_work_merged, chunk_room)) return rc;      // (an overflowing cut leaves ranges behind the table: not read)
        if (int rc = devfin_headers(ds, *d, rbase)) return rc;     // (the 16-byte headers with linear positions: wide kernel, padding, host mapping -- behind everything the first pass waits for)
    }

    fin_trace("merged groups");
    return MSNV_OK;
}

// ---- columns
int Finalize::columns() {
    d->n_reads = rbase[S]; d->n_seq_bytes = sbase[S]; d->n_blk = bbase[S];
    if (!R.fast) if (int rc = dev_alloc((void **)&d->hdr, (rbase[S] + 1) * sizeof(ReadHdr), &d->device_bytes)) return rc;
    if (!R.dense && !HDR4) if (int rc = dev_alloc((void **)&d->hdr8, (rbase[S] + 1) * sizeof(PieceHdr), &d->device_bytes)) return rc;
    if (!R.dense && HDR4 && !R.fast) if (int rc = dev_alloc((void **)&d->hdr4, (rbase[S] + 4) * sizeof(uint32_t), &d->device_bytes)) return rc;
    if (R.dense) if (int rc = dev_alloc((void **)&d->blk, (bbase[S] + 1) * sizeof(uint32_t), &d->device_bytes)) return rc;
    R.cols_on_device = R.fast && !R.dense;
    if (R.cols_on_device) { if (int rc = devpack_place_columns(ds, *d, sbase)) return rc; }
    else {
        if (int rc = dev_alloc((void **)&d->seq, sbase[S] + 256, &d->device_bytes)) return rc;     // lanes past the end of the last piece read on
        if (int rc = dev_memset(d->seq, 0xff, sbase[S] + 256)) return rc;                          // (the < 16 bytes between two samples' columns: defined, so that two builds of a dataset can be compared)
        // the quality column of the device is ONE BIT per base -- "below the -Q cutoff" -- at the index of the base's nibble in the seq column: the
        // cutoff is a parameter of the dataset (mpileup -Q, metaSNV.py:160-165 never changes it) and nothing else of a quality is ever looked at
        // behind the overlap tweak and the token limit, which ran on the host (pass 1 above).  1 B -> 1/8 B per base of HBM and of upload.
        if (int rc = dev_alloc((void **)&d->qual, sbase[S] / 4 + 64, &d->device_bytes)) return rc;
        if (int rc = dev_memset(d->qual, 0, sbase[S] / 4 + 64)) return rc;
    }
    d->qlow_cutoff = ds.params.min_baseq;
    uint64_t alg = 0;
    fin_trace("  column allocs + memsets");
    // the samples' columns go up from a few host threads at a time (a pageable copy is staged by the runtime: several in flight keep
    // the link busy while the compact headers of the next samples are built)
    const size_t n_up = std::min<size_t>(S, std::min<size_t>(8, msnv_default_threads()));
    std::vector<std::thread> th;
    if (R.cols_on_device) upload_columns();                        // (nothing to upload: no threads)
    else for (size_t t = 0; t < n_up; ++t) th.emplace_back([this]() { upload_columns(); });
    for (auto &t : th) t.join();
    if (up_err.load()) return fail(up_err.load(), "%s", up_msg.c_str());
    fin_trace("  column copies");
    {   // device-packed samples: the alignment padding behind their pieces, then their round buffers and the pack tables go back
        on_dev.assign(S, 0);
        for (size_t s = 0; s < S; ++s) on_dev[s] = ds.samples[s].on_device ? 1 : 0;
        // (round 6: the device pack's emit kernels leave the padding in place -- the pass over every piece is only taken when a FASTA record
        // is longer than its contig, where "the reference" behind the contig's last tile position differs between the two)
        bool fasta_longer = false;
        for (size_t c = 0; c < NC; ++c) if (ds.sel[c] && ds.has_seq[c] && (int64_t)ds.seqs[c].size() > maxend[c]) fasta_longer = true;
        if (!R.dense && (!ds.dp.pad_in_emit || fasta_longer || knob::fill_padding())) if (int rc = devpack_fill_padding(*d, on_dev, stream)) return rc;
    }
    for (size_t s = 0; s < S; ++s) {
        const SampleCols &sc = ds.samples[s];
        ds.info.bytes_headers += R.dense ? (bbase[s + 1] - bbase[s]) * sizeof(uint32_t) : (rbase[s + 1] - rbase[s]) * (HDR4 ? sizeof(uint32_t) : sizeof(PieceHdr));
        ds.info.bytes_cigar += sc.alg_cigar_bytes;
        alg += sc.alg_8d_bytes;
        ds.info.bytes_seq += sc.alg_seq_bytes;
        ds.info.bytes_qual += sc.alg_qual_bytes;
    }
    d->algorithmic_bytes = alg;                  // SURVEY.md section 8d figure; the shipped bytes are bytes_headers + bytes_seq + bytes_qual
    fin_trace("columns");
    return MSNV_OK;
}

void Finalize::upload_columns() {
    (void)dev_set_device(device);
    std::vector<uint8_t> qbits;
    for (;;) {
        const size_t s = up_next.fetch_add(1);
        if (s >= S || up_err.load()) break;
        SampleCols &sc = ds.samples[s];
        int rc = R.fast ? MSNV_OK : dev_upload(d->hdr + rbase[s], sc.hdr.data(), sc.hdr.size() * sizeof(ReadHdr));
        if (R.fast) {
            // (headers and 4-byte headers were built in HBM; so were the block descriptors of the dense layout)
            if (R.dense) rc = devpack_copy_blocks(sc, d->blk + bbase[s], stream);
        } else if (!rc && R.dense) {
            rc = dev_upload(d->blk + bbase[s], sc.blk.data(), sc.blk.size() * sizeof(uint32_t));
        } else if (!rc && HDR4) {
            rc = dev_upload(d->hdr4 + rbase[s], hdr4_of[s].data(), hdr4_of[s].size() * sizeof(uint32_t));
            std::vector<uint32_t>().swap(hdr4_of[s]);
        } else if (!rc) {   // compact tile-local headers of the narrow kernel: {start in tile | length << 11, seq offset / SEQ_ALIGN}
            std::vector<PieceHdr> h8(sc.hdr.size());
            for (size_t i = 0; i < sc.hdr.size(); ++i) h8[i] = PieceHdr{(sc.hdr[i].gpos % TILE) | sc.hdr[i].cig << 11, sc.hdr[i].seqoff >> SEQ_ALIGN_LOG2};
            rc = dev_upload(d->hdr8 + rbase[s], h8.data(), h8.size() * sizeof(PieceHdr));
        }
        if (R.cols_on_device) {}                                     // (placed above, round by round)
        else if (!rc && sc.on_device) rc = devpack_copy_columns(sc, d->seq + sbase[s], d->qual + sbase[s] / 4, stream);      // packed on the device: HBM to HBM
        else {
            if (!rc) rc = dev_upload(d->seq + sbase[s], sc.seq.data(), sc.seq.size());
            if (!rc) {
                pack_lowq(sc.qual.data(), sc.qual.size(), ds.params.min_baseq, qbits);
                rc = dev_upload(d->qual + sbase[s] / 4, qbits.data(), qbits.size());      // (sbase: multiples of 16 bytes of seq = 32 flags)
            }
        }
        if (rc) { std::lock_guard<std::mutex> lk(up_mu); if (!up_err.load()) { up_msg = msnv_last_error(); up_err.store(rc); } continue; }
        // release host staging of the bulky columns; headers stay (coverage pass, results mapping)
        std::vector<uint8_t>().swap(sc.seq);
        std::vector<uint8_t>().swap(sc.qual);
        if (R.dense) std::vector<uint32_t>().swap(sc.blk);
    }
}

// ---- intermediates (before the coverage index: their allocations and fills -- queued on the context's stream, in front of the first
// pass -- run while the device still works on the index; the coverage index holds finalize's last wait)
int Finalize::intermediates() {
    double est_events = 0.0;                                        // mismatching bases the sampled rate predicts: what the event list is sized by
    {
        // Allele bookkeeping of the narrow work items.  Clean reads (the benchmark's 0.1 % errors): a mismatching base is an EVENT -- one
        // memory-side atomic on the position's totals + 8 bytes in the event list, scattered into the called sites' cells afterwards.
        // At a few per cent of mismatches (real metagenomic reads against a species representative) every position carries some and the
        // events are the pass: 37.7 M of them at 3 % = 1.2 ms of atomics in the pileup kernel + 1.5 ms of scatter (profiles/r03e).  Then
        // the alleles go the way the coverage goes: every (sample, tile) pair writes four byte PLANES (A, C, G, T counts per position,
        // 8 KB a pair, plain 16-byte stores), the gate kernel sums the planes, the gather transposes them into the cells.  Picked when the
        // sampled mismatch rate reaches 1.0 % (with byte qualities the break-even was 1.5 %; the kernel that reads one bit of quality per base
        // no longer hides the events behind HBM time: at 0.6 % of errors -- 0.85 % sampled with the cohort's SNVs -- events 0.603 vs planes
        // 0.643 ms a pass, at 1 % -- 1.25 % sampled -- 0.773 vs 0.601 ms, profiles/r03zam_crossover.txt; at 3 % 3.55 vs 2.08 ms, at 10 % 8.5 vs
        // 2.1 ms, profiles/r03g_*; a cost model in events per pair put the sigma = 2 cohort -- 0.4 % of mismatches, deep
        // pairs -- on planes, where the five-plane gather over its 526 k sites cost more than the events: 4.95 vs 4.08 ms);
        // MSNV_ALLELES=planes | events overrides.
        // Needs byte counts everywhere: not with wide work items (MSNV_DEEP=wide) and not in the dense piece layout's kernel.
        if (int rc = devpack_sync_pending(ds)) return rc;               // (the last round's mismatch sample: its kernels were left running behind the pack)
        uint64_t sb = 0, sm = 0;
        for (const SampleCols &sc : ds.samples) { sb += sc.mm_sampled_bases; sm += sc.mm_sampled; }
        const double rate = sb ? (double)sm / (double)sb : 0.0;
        est_events = rate * (double)tot_bases;
        bool planes = rate >= 0.010;
        if (const char forced = knob::alleles()) planes = forced == 'p';
        if (R.dense || d->n_work > d->n_work_narrow + d->n_work_merged || pairs.empty()) planes = false;
        d->allele_planes = planes;
        ds.info.allele_planes = planes ? 1 : 0;
        ds.info.sampled_mismatch_ppm = (uint64_t)(rate * 1e6);
    }
    // sparse buffers: generous first guess, grown on MSNV_ECAPACITY by the caller
    // (the event list: four times the mismatching bases the sample of every 16th piece predicts, at most one per 16 bases -- the flat
    // "one per 16 bases" of the earlier rounds was 29 GB of HBM, and 1 s of hipMalloc, for BASELINE configs[2]'s 5.8e10 bases at 0.4 % of mismatches)
    d->cap_events = knob::cap_events((uint32_t)std::min<uint64_t>(0x7fffffffull, std::max<uint64_t>(1u << 20, std::min<uint64_t>(tot_bases / 16, (uint64_t)(4.0 * est_events) + (1u << 20)))), EV_LISTS);   // (tests force the grow-and-rerun path)
    d->cap_overflow = (uint32_t)std::min<uint64_t>(0x7fffffffull, std::max<uint64_t>(1u << 16, npos / 8));
    d->cap_sites = (uint32_t)std::min<uint64_t>(0x7fffffffull, std::max<uint64_t>(1u << 16, npos / 4));
    for (const TilePair &tp : pairs) if ((tp.pad & 0xffu) == 1) { d->any_split = true; break; }
    if (int rc = passbufs_alloc(*d, *d, *d, stream)) return rc;      // (the output columns come with the first pass: their capacities are still 0)

    ds.info.n_samples = S; ds.info.n_contigs = 0; ds.info.n_positions = 0;
    for (size_t c = 0; c < NC; ++c) if (ds.sel[c]) { ds.info.n_contigs++; ds.info.n_positions += (uint64_t)ds.lengths[c]; }
    ds.info.n_reads = tot_reads; ds.info.n_reads_pileup = tot_pile_reads; ds.info.n_pileup_bases = tot_bases;
    ds.info.n_tiles = nt; ds.info.n_pairs = pairs.size(); ds.info.n_work = work.size();
    fin_trace("intermediates");
    return MSNV_OK;
}

// ---- the coverage index's tables: joined (device-packed datasets: built beside everything above) or built here
int Finalize::coverage_index_up() {
    if (cov_job.th.joinable()) { if (int rc = cov_job.join()) return rc; }
    else if (int rc = coverage_tables(cov_arena, false)) return rc;
    fin_trace("    cov tables: staged");
    if (int rc = cov_arena.commit(*d)) return rc;
    fin_trace("    cov tables: up");
    {   // accumulator copies: as many as fit 64 MB, at most 8 (many contigs = few tiles per contig = little contention anyway)
        d->n_cov_rows = ds.cov_row_sample.size();
        ds.cov_row_scanned_ok = false;
        const uint64_t acc_bytes = std::max<uint64_t>(1, d->n_cov_rows) * (1 + COV_BINS) * sizeof(unsigned long long);
        d->cov_copies = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8, (64ull << 20) / std::max<uint64_t>(1, acc_bytes)));
        if (int rc = dev_alloc((void **)&d->cov_acc, d->cov_copies * acc_bytes, &d->device_bytes)) return rc;
    }
    fin_trace("  coverage tables");
    return MSNV_OK;
}

// ---- the last wait: how many chunks the narrow items got (cut in HBM, counted there; an event behind the cut's kernels)
int Finalize::last_wait() {
    if (R.chunks_on_device) {
        uint64_t n_narrow = 0; bool overflow = false;
        if (int rc = devfin_chunks_result(ds, &n_narrow, &overflow)) return rc;
        if (overflow) {
            // (more chunks than the bound gave room for: once more with the exact number, which is known now; the first table's bytes
            // leave the dataset's count with it, the new table's come in with its dev_alloc)
            d->device_bytes -= (M + chunk_cap + 1) * sizeof(ChunkDesc);
            if (int rc = dev_stream_wait(stream)) return rc;              // (kernels still queued read the first table: msnv_fin_work_first)
            dev_free(d->chunks); d->chunks = nullptr;
            if (M + n_narrow > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 chunks in one shard");
            if (int rc = dev_alloc((void **)&d->chunks, (M + n_narrow + 1) * sizeof(ChunkDesc), &d->device_bytes)) return rc;
            if (int rc = dev_upload(d->chunks, mchunks.data(), M * sizeof(ChunkDesc))) return rc;
            if (int rc = devfin_chunks_launch(ds, *d, narrow_pairs, item_first, (uint32_t)M, n_narrow)) return rc;
            if (int rc = devfin_work_first(ds, *d, d->n_work_narrow + d->n_work_merged, M + n_narrow)) return rc;
            if (int rc = dev_stream_wait(stream)) return rc;
            if (int rc = devfin_chunks_result(ds, &n_narrow, &overflow)) return rc;
            if (overflow) return fail(MSNV_EINVAL, "internal: the chunk count changed between two cuts of the same pairs");
            fin_trace("chunks: cut again with the exact count");
        }
        d->n_chunks = M + n_narrow;
    }
    if (int rc = devpack_finish(ds)) return rc;                // (device-packed samples: the rounds' buffers and the pack tables go back)
    fin_trace("pack tables released");
    ds.info.bytes_index = pairs.size() * sizeof(TilePair) + work.size() * sizeof(WorkItem) + d->n_chunks * sizeof(ChunkDesc) + (nt + 1) * 4;
    ds.info.device_bytes = d->device_bytes;
    ds.finalized = true;
    return MSNV_OK;
}
}  // namespace

int finalize_dataset(msnv_dataset &ds) {
    if (ds.samples.empty()) return fail(MSNV_EINVAL, "dataset has no samples");
    if (ds.samples.size() >= 16384) return fail(MSNV_EDOMAIN, "more than 16383 samples per dataset are not supported");
    // MSNV_FINALIZE_TRACE=1: wall seconds of every stage to stderr (where a big dataset's finalize goes)
    fin_trace_reset();
    Finalize F(ds);
    int rc = F.decide_route();
    if (!rc) rc = F.tile_layout();
    if (!rc) rc = F.launch_coverage();
    if (!rc) rc = F.reference();
    if (!rc) rc = F.callable_ranges();
    if (!rc) rc = F.layout_samples();
    if (!rc) rc = F.pairs_per_sample();
    if (!rc) rc = F.pair_csr();
    if (!rc) rc = F.pair_classes();
    if (!rc) rc = F.slots();
    if (!rc) rc = F.work_list();
    if (!rc) rc = F.partial_rows();
    if (!rc) rc = F.merged_chunks();
    if (!rc) rc = F.narrow_chunks();
    if (!rc) rc = F.upload_index();
    if (!rc) rc = F.columns();
    if (!rc) rc = F.intermediates();
    if (!rc) rc = F.coverage_index_up();
    if (!rc) rc = F.last_wait();
    return rc;
}

}  // namespace msnv
