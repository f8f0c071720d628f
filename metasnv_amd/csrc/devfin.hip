// metasnv_amd/csrc/devfin.hip -- finalize's device side: the per-piece and per-interval parts of finalize_dataset (finalize.cpp) as kernels,
// for a dataset whose samples were all packed on the device (devpack.hip).
//
// What it replaces: the host loops of finalize.cpp over every piece and every qaCompute interval (qaCompute.cpp:530-552 cuts them) -- the tile
// index's chunk descriptors and piece headers, the genome coverage index, the re-layouts of deep runs and of short reads.  The headers and
// intervals stay in HBM where the rounds left them; the host works on (sample, tile) pairs only.  Every function mirrors the host loop named
// beside it and produces the same bytes (tests/test_gpu_devpack.py compares every table of the two builds; tests/test_gpu_finalize_routes.py
// takes every route below).
//
// Stages in call order, the stage of `Finalize` (finalize.cpp) that calls each beside it:
//   devfin_deep_runs         decide_route       msnv_fin_deep_sweep: exact depth of the deep (sample, tile) runs, the really deep ones dealt into groups;
//                                               msnv_fin_deep_perm, the round's gather (devpack.hip), msnv_fin_stored / msnv_fin_relayout: headers
//                                               group by group, the sample's columns in header order
//   devfin_overhang          tile_layout        the per-contig maxima of reads that run past their contig (a copy)
//   devfin_coverage_launch   launch_coverage    the coverage index's kernels ahead of their results (CovIndex::launch_ahead: msnv_fin_cov_emit_dense,
//                                               _dense_flags, _dense_runs; the pair tables' counts: msnv_cov_flags_t, _count_items, _rows, _counts)
//   devfin_coverage          coverage_tables    collects them (CovIndex::collect; msnv_cov_write_pairs / _items write the pair tables) -- or runs the
//                                               index there, waiting: the late dense route, the sort form (msnv_fin_cov_measure, msnv_fin_cov_emit,
//                                               msnv_fin_pair_flags, msnv_fin_cov_runs)
//   devfin_dense             layout_samples     short reads as dense block streams: msnv_fin_dense_count, _place, _copy
//   devfin_chunks_launch     upload_index       the narrow pairs' chunks without a wait: msnv_fin_chunks<false>, a scan, msnv_fin_chunks<true>,
//                                               msnv_fin_work_chunks; again from last_wait behind an overflow
//   devfin_merged_headers    upload_index       msnv_fin_merged: the merged groups' 8-byte piece headers
//   devfin_work_first        upload_index       msnv_fin_work_first: every work item's first chunk descriptor into the item
//   devfin_headers           upload_index       msnv_fin_headers: the 16-byte headers with linear positions
//   devpack_place_columns    columns            the rounds' columns adopted or copied (devpack_copy_columns; devpack_copy_blocks for the dense layout)
//   devpack_fill_padding     columns            msnv_fill_padding, when the emit kernels did not leave the padding nibbles
//   devfin_chunks_result     last_wait          the cut's two pinned words, behind its event
//   devpack_finish           last_wait          the last waits; the pack's buffers and finalize's own (devfin_release) go back
// State between the calls: DevPackTables::Fin (dataset.h); the small results come to the host through FinWords (devfin.h).
// Buffers are carved from one block each by Carve / carve_block; what both device files share is devwork.h.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "devfin.h"
#include "devwork.h"

namespace msnv {

// The two rocPRIM forms that only finalize uses (devwork.h: Prim)
int Prim::scan64(const uint32_t *in, unsigned long long *out, size_t n) { return exclusive(in, out, 0ull, n, rocprim::plus<unsigned long long>()); }
int Prim::reserve_scan32(size_t n) {
    size_t need = 0;
    if (int rc = exclusive((const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n, rocprim::plus<uint32_t>(), &need)) return rc;
    return room(need + 256);
}
namespace {

__global__ void msnv_fin_headers(const ReadHdr *src, const int32_t *tid, unsigned long long n, const uint32_t *tile_base, ReadHdr *dst) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ReadHdr h = src[i];
    h.gpos += tile_base[tid[i]] * TILE;                           // contig-relative -> linear position of the shard
    dst[i] = h;
}

// chunks of the narrow work items' pairs (finalize.cpp: "chunk descriptors of the narrow work items", HDR4 form): up to CHUNK_READS consecutive
// pieces whose seq bytes lie within 2^HDR4_OFF_BITS alignment units of the chunk's lowest offset; FILL writes the descriptors and the
// 4-byte chunk-relative piece headers.  One WAVEFRONT per pair: 64 pieces a step, the greedy rule's running minimum / maximum as prefix
// scans over the lanes, the first piece that would stretch the chunk too far found by a ballot (a thread per pair walking ~250 headers
// one after the other was 1.1 ms of finalize on the benchmark shape).
__device__ __forceinline__ unsigned long long wave_prefix_min(unsigned long long v) {
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(v, o); if ((int)(threadIdx.x & 63u) >= o) v = y < v ? y : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_prefix_max(unsigned long long v) {
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(v, o); if ((int)(threadIdx.x & 63u) >= o) v = y > v ? y : v; }
    return v;
}
template <bool FILL>
__global__ __launch_bounds__(256) void msnv_fin_chunks(const TilePair *pairs, const uint32_t *list, uint32_t n, const ReadHdr *const *s_hdr, const unsigned long long *rbase, const unsigned long long *sbase,
                                                       uint32_t *counts, const uint32_t *chunk_base, ChunkDesc *chunks, uint32_t *hdr4, uint32_t chunk_cap) {
    const uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (j >= n) return;
    const uint32_t k = list[j];
    const TilePair p = pairs[k];
    // (the sample's headers where the pack's round left them: positions contig-relative, which is all the same inside a tile -- contigs start
    // on tile boundaries --, so nothing here waits for the linear copy, msnv_fin_headers)
    const ReadHdr *h = s_hdr[p.sample];
    constexpr unsigned long long span_max = (unsigned long long)SEQ_ALIGN << HDR4_OFF_BITS;
    uint32_t r = p.read_lo, c = 0;
    while (r < p.read_hi) {
        // the chunk that starts at r: pieces r .. e - 1
        unsigned long long lo = ~0ull, hi = 0;                    // of the pieces taken so far (wave-uniform)
        uint32_t e = r;
        ReadHdr mine[CHUNK_READS / 64];
#pragma unroll
        for (uint32_t step = 0; step < CHUNK_READS / 64; ++step) {
            const uint32_t i = r + 64u * step + lane;
            const bool have = i < p.read_hi;
            if (have) mine[step] = h[i];
            if (e != r + 64u * step) continue;                     // (the chunk was closed inside an earlier step; wave-uniform)
            const unsigned long long o = have ? (unsigned long long)mine[step].seqoff : 0ull;
            unsigned long long pmin = wave_prefix_min(have ? o : ~0ull), pmax = wave_prefix_max(have ? o : 0ull);
            pmin = pmin < lo ? pmin : lo; pmax = pmax > hi ? pmax : hi;
            const unsigned long long stop = __ballot(!have || pmax - pmin >= span_max);      // first lane that does not join
            const uint32_t take = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
            if (take) { lo = __shfl(pmin, (int)take - 1); hi = __shfl(pmax, (int)take - 1); }
            e += take;
        }
        if (e == r) e = r + 1;                                     // (a single piece always fits: its span is 0 -- never taken, kept against a stuck loop)
        if (FILL) {
#pragma unroll
            for (uint32_t step = 0; step < CHUNK_READS / 64; ++step) {
                const uint32_t i = r + 64u * step + lane;
                if (i < e) hdr4[rbase[p.sample] + i] = (mine[step].gpos % TILE) | mine[step].cig << 11 | (uint32_t)((mine[step].seqoff - lo) >> SEQ_ALIGN_LOG2) << 19;
            }
            if (lane == 0 && chunk_base[j] + c < chunk_cap) chunks[chunk_base[j] + c] = ChunkDesc{rbase[p.sample] + r, sbase[p.sample] + lo, p.pad >> 8, k, (e - r) | (e >= p.read_hi ? 1u << 16 : 0u), p.pad & 0xffu};
        }
        ++c; r = e;
    }
    if (!FILL && lane == 0) counts[j] = c;
}
// The narrow work items' chunk ranges from the scanned counts, on the device (round 6: the host used to wait for the scan to write them):
// item wi owns the listed pairs [item_first[wi], item_first[wi + 1]) and with them the chunks [base + scan[..], base + scan[..]).  The total
// and "more chunks than there is room for" go to the host through pinned words; it looks at them behind finalize's last wait.
__global__ void msnv_fin_work_chunks(WorkItem *work, uint32_t n_narrow, const uint32_t *item_first, const uint32_t *scan, uint32_t n_listed, uint32_t base, uint32_t cap, uint32_t *result) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { result[0] = scan[n_listed]; result[1] = scan[n_listed] > cap ? 1u : 0u; }
    if (i >= n_narrow) return;
    work[i].chunk_lo = base + scan[item_first[i]];
    work[i].chunk_hi = base + scan[item_first[i + 1]];
}
// every narrow / merged work item's first chunk descriptor, copied into the item (kernels.hip: a workgroup starts loading without the descriptor stream)
// (n_room: descriptors the table holds -- after an overflow of the device's cut the items' ranges point behind it until finalize cuts again)
__global__ void msnv_fin_work_first(WorkItem *work, uint32_t n, const ChunkDesc *chunks, unsigned long long n_room) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (work[i].chunk_hi > work[i].chunk_lo && work[i].chunk_lo < n_room) work[i].first = chunks[work[i].chunk_lo];
}

__global__ void msnv_fin_merged(const TilePair *pairs, const DevMergedSrc *list, uint32_t n, const ReadHdr *const *s_hdr, const unsigned long long *sbase, PieceHdr *hm) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DevMergedSrc m = list[j];
    const TilePair p = pairs[m.pair];
    const ReadHdr *h = s_hdr[p.sample];                            // (contig-relative positions: only the tile-relative part is used)
    for (uint32_t r = p.read_lo; r < p.read_hi; ++r) {
        const unsigned long long so = (sbase[p.sample] + h[r].seqoff) >> SEQ_ALIGN_LOG2;     // 37 bits: bits 32-36 ride in bits 27-31 of the first word
        hm[m.h_base + (r - p.read_lo)] = PieceHdr{(h[r].gpos % TILE) | h[r].cig << 11 | m.in_group << 19 | (uint32_t)(so >> 32) << 27, (uint32_t)so};
    }
}

// qaCompute's intervals -> the coverage kernel's inputs (finalize.cpp: "genome coverage index")
__device__ __forceinline__ uint32_t sample_of(const unsigned long long *iv_start, uint32_t n_samples, unsigned long long j) {
    uint32_t a = 0, b = n_samples;
    while (b - a > 1) { const uint32_t m = (a + b) / 2; if (iv_start[m] <= j) a = m; else b = m; }
    return a;
}
__global__ void msnv_fin_cov_measure(const int32_t *ctid, const int32_t *cbeg, const int32_t *cend, unsigned long long n, const DpContig *ctg, const uint32_t *tile_base,
                                     uint32_t *keep, uint32_t *ntile) {
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t c = ctid[j];
    const long long L = ctg[c].len, b = cbeg[j];
    const bool minus_one = b > (long long)cend[j];                                          // {L, L - 1}: "-1 at L - 1" (msnv_emit_headers)
    const long long e = minus_one ? (long long)cend[j] : ((long long)cend[j] >= L ? L - 1 : (long long)cend[j]);      // qaCompute.cpp:544-549
    const bool k = minus_one || b < e;
    uint32_t nt = 0;
    if (k) {
        const unsigned long long g0 = (unsigned long long)tile_base[c] * TILE;
        const uint32_t tf = (uint32_t)((g0 + (unsigned long long)(minus_one ? e : b)) / TILE), tl = minus_one ? tf : (uint32_t)((g0 + (unsigned long long)e - 1) / TILE);
        nt = tl - tf + 1;
    }
    keep[j] = k ? 1u : 0u; ntile[j] = nt;
}
// (the round's arrays are indexed by j, the dataset-wide ones -- kidx, iv_start -- by j0 + j; ntile / ebase come offset to the round)
__global__ void msnv_fin_cov_emit(const int32_t *ctid, const int32_t *cbeg, const int32_t *cend, unsigned long long n, unsigned long long j0, const DpContig *ctg,
                                  const uint32_t *tile_base, const unsigned long long *iv_start, uint32_t n_samples, const uint32_t *ntile, const uint32_t *kidx_all,
                                  const uint32_t *ebase, Pair32 *iv, unsigned long long *ekey, uint32_t *eval) {
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !ntile[j]) return;
    const uint32_t *kidx = kidx_all + j0;
    const int32_t c = ctid[j];
    const long long L = ctg[c].len, b = cbeg[j];
    const bool minus_one = b > (long long)cend[j];
    const long long e = minus_one ? (long long)cend[j] : ((long long)cend[j] >= L ? L - 1 : (long long)cend[j]);
    const unsigned long long g0 = (unsigned long long)tile_base[c] * TILE;
    iv[kidx[j]] = Pair32{(uint32_t)(g0 + (unsigned long long)b), (uint32_t)(g0 + (unsigned long long)e)};
    const uint32_t s = sample_of(iv_start, n_samples, j0 + j);
    const uint32_t idx = kidx[j] - kidx_all[iv_start[s]];                                   // index among the sample's kept intervals
    const uint32_t tf = (uint32_t)((g0 + (unsigned long long)(minus_one ? e : b)) / TILE), tl = minus_one ? tf : (uint32_t)((g0 + (unsigned long long)e - 1) / TILE);
    unsigned long long w = ebase[j];
    for (uint32_t t = tf; t <= tl; ++t, ++w) { ekey[w] = (unsigned long long)s << 32 | t; eval[w] = idx; }
}
__global__ void msnv_fin_cov_runs(const unsigned long long *skey, const uint32_t *sval, const uint32_t *flag, const uint32_t *rid_incl, unsigned long long n, DevCovPair *out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rid_incl[i] - 1u;
    if (flag[i]) { out[r].tile = (uint32_t)skey[i]; out[r].sample = (uint32_t)(skey[i] >> 32); out[r].lo = sval[i]; }
    if (i + 1 == n || flag[i + 1]) out[r].hi = sval[i] + 1u;                                  // (stable sort: the run's values ascend)
}
// The (sample, tile) runs without a sort: the intervals of a sample come in nearly ascending order, so a run is the RANGE [first, last + 1)
// of the kept intervals that touch the tile -- a minimum and a maximum per (sample, tile), kept in a dense [sample][tile] table when that
// table is small beside the interval list (else the sort of (sample, tile, index) entries above).  Consecutive lanes hold consecutive
// intervals, nearly always of one (sample, tile): the first lane of such a stretch carries its minimum, the last its maximum -- two atomics
// per stretch instead of two per interval; an interval that touches several tiles adds to the other tiles' entries by itself.
__global__ __launch_bounds__(256) void msnv_fin_cov_emit_dense(const int32_t *ctid, const int32_t *cbeg, const int32_t *cend, unsigned long long n, unsigned long long j0, const DpContig *ctg,
                                                               const uint32_t *tile_base, const unsigned long long *iv_start, uint32_t n_samples, const uint32_t *keep_all, const uint32_t *kidx_all,
                                                               uint32_t n_tiles, Pair32 *iv, uint32_t *lo, uint32_t *hi) {
    const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = ~0ull; uint32_t idx = 0, tf = 0, tl = 0, s = 0;
    if (j < n && (!keep_all || keep_all[j0 + j])) {
        const int32_t c = ctid[j];
        const long long L = ctg[c].len, b = cbeg[j];
        const bool minus_one = b > (long long)cend[j];
        const long long e = minus_one ? (long long)cend[j] : ((long long)cend[j] >= L ? L - 1 : (long long)cend[j]);
        const unsigned long long g0 = (unsigned long long)tile_base[c] * TILE;
        const uint32_t place = keep_all ? kidx_all[j0 + j] : (uint32_t)(j0 + j);          // (no tables: every interval is kept -- the device pack writes no other since round 6)
        iv[place] = Pair32{(uint32_t)(g0 + (unsigned long long)b), (uint32_t)(g0 + (unsigned long long)e)};
        s = sample_of(iv_start, n_samples, j0 + j);
        idx = place - (keep_all ? kidx_all[iv_start[s]] : (uint32_t)iv_start[s]);
        tf = (uint32_t)((g0 + (unsigned long long)(minus_one ? e : b)) / TILE); tl = minus_one ? tf : (uint32_t)((g0 + (unsigned long long)e - 1) / TILE);
        key = (unsigned long long)s * n_tiles + tf;
    }
    const unsigned long long kp = __shfl_up(key, 1), kn = __shfl_down(key, 1);
    const uint32_t lane = threadIdx.x & 63u;
    if (key != ~0ull) {
        if (lane == 0 || kp != key) atomicMin(&lo[key], idx);
        if (lane == 63 || kn != key) atomicMax(&hi[key], idx + 1u);
        for (uint32_t t = tf + 1; t <= tl; ++t) { atomicMin(&lo[(unsigned long long)s * n_tiles + t], idx); atomicMax(&hi[(unsigned long long)s * n_tiles + t], idx + 1u); }
    }
}
__global__ void msnv_fin_cov_dense_flags(const uint32_t *hi, unsigned long long n, uint32_t *flag) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = (i < n && hi[i]) ? 1u : 0u;
}
__global__ void msnv_fin_cov_dense_runs(const uint32_t *lo, const uint32_t *hi, const uint32_t *rid_excl, unsigned long long n, uint32_t n_tiles, DevCovPair *out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !hi[i]) return;
    out[rid_excl[i]] = DevCovPair{(uint32_t)(i % n_tiles), (uint32_t)(i / n_tiles), lo[i], hi[i]};
}
// ---- the coverage index's pair tables on the device (round 6; finalize.cpp: cov_index built them on the host behind finalize's last wait, 0.5 ms of
// loops over the (sample, tile) runs on the benchmark shape).  The dense [sample][tile] table read TILE-major gives the pairs in their final
// order (tiles ascending, samples ascending inside a tile) by one scan of its flags; the accumulator rows -- one per (sample, contig) that has
// intervals -- by a scan of a presence table; the work items (finalize.cpp's cut: COV_ITEM_PAIRS pairs, or fewer when one pair alone is deep) by a
// thread per tile, counted first, written once the host has allocated the tables from the counts that come back with the index's own.
__global__ void msnv_cov_flags_t(const uint32_t *hi, uint32_t n_samples, uint32_t n_tiles, const uint32_t *tcont, uint32_t n_contigs, uint32_t *flag_t, uint32_t *pres) {
    const unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, n = (unsigned long long)n_samples * n_tiles;
    if (k > n) return;
    uint32_t f = 0;
    if (k < n) {
        const uint32_t t = (uint32_t)(k / n_samples), sm = (uint32_t)(k % n_samples);
        f = hi[(unsigned long long)sm * n_tiles + t] ? 1u : 0u;
        if (f) pres[(unsigned long long)sm * n_contigs + tcont[t]] = 1u;
    }
    flag_t[k] = f;
}
// (a WAVEFRONT per tile: its lanes ask for 64 samples' table entries at once, the cut -- sequential over the pairs -- runs over them by shuffles.
// First form: a thread per tile with a loop over the samples, 61 us for the benchmark's 440 tiles x 160 samples: a chain of loads per thread)
__global__ __launch_bounds__(64) void msnv_cov_count_items(const uint32_t *lo, const uint32_t *hi, uint32_t n_samples, uint32_t n_tiles, uint32_t item_intervals, uint32_t narrow_max, uint32_t *n_item, uint32_t *wide) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t > n_tiles) return;
    uint32_t items = 0;
    if (t < n_tiles) {
        unsigned long long acc = 0; uint32_t in_item = 0; bool w = false;
        for (uint32_t base = 0; base < n_samples; base += 64u) {
            const uint32_t sm = base + lane;
            uint32_t span = 0; bool has = false;
            if (sm < n_samples) {
                const uint32_t h = hi[(unsigned long long)sm * n_tiles + t];
                if (h) { has = true; span = h - lo[(unsigned long long)sm * n_tiles + t]; }
            }
            w |= has && span > narrow_max;
            unsigned long long m = __ballot(has);
            while (m) {                                                  // (uniform: every lane keeps the same cut state)
                const int k = __builtin_ctzll(m);
                m &= m - 1ull;
                acc += __shfl(span, k); ++in_item;
                if (acc >= item_intervals || in_item >= COV_ITEM_PAIRS) { ++items; acc = 0; in_item = 0; }
            }
        }
        if (in_item) ++items;
        if (__any(w) && lane == 0) *wide = 1u;
    }
    if (lane == 0) n_item[t] = items;
}
__global__ void msnv_cov_rows(const uint32_t *pres, const uint32_t *rowid, uint32_t n_samples, uint32_t n_contigs, uint32_t *row_sample, uint32_t *row_contig, uint32_t *row_start) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, n = (unsigned long long)n_samples * n_contigs;
    if (i > n) return;
    if (i < n && pres[i]) { row_sample[rowid[i]] = (uint32_t)(i / n_contigs); row_contig[rowid[i]] = (uint32_t)(i % n_contigs); }
    if (i % n_contigs == 0u || i == n) row_start[i / n_contigs] = rowid[i];            // (entry n_samples: the rows in all)
}
__global__ void msnv_cov_counts(const uint32_t *rid_t, unsigned long long n_tab, const uint32_t *rowid, unsigned long long n_sc, const uint32_t *item_off, uint32_t n_tiles, const uint32_t *wide, uint32_t *out) {
    if (blockIdx.x || threadIdx.x) return;
    out[0] = rid_t[n_tab]; out[1] = rowid[n_sc]; out[2] = item_off[n_tiles]; out[3] = *wide;
}
__global__ void msnv_cov_write_pairs(const uint32_t *lo, const uint32_t *hi, const uint32_t *rid_t, const uint32_t *rowid, const uint32_t *tcont, const unsigned long long *iv_start,
                                     uint32_t n_samples, uint32_t n_tiles, uint32_t n_contigs, TilePair *pairs) {
    const unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, n = (unsigned long long)n_samples * n_tiles;
    if (k >= n) return;
    const uint32_t t = (uint32_t)(k / n_samples), sm = (uint32_t)(k % n_samples);
    const uint32_t h = hi[(unsigned long long)sm * n_tiles + t];
    if (!h) return;
    const unsigned long long b = iv_start[sm];
    pairs[rid_t[k]] = TilePair{sm, lo[(unsigned long long)sm * n_tiles + t], h, rowid[(unsigned long long)sm * n_contigs + tcont[t]], (uint32_t)b, (uint32_t)(b >> 32), 0u, 0u};
}
__global__ __launch_bounds__(64) void msnv_cov_write_items(const TilePair *pairs, const uint32_t *rid_t, const uint32_t *item_off, uint32_t n_samples, uint32_t n_tiles, uint32_t item_intervals, WorkItem *work) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t p0 = rid_t[(unsigned long long)t * n_samples], p1 = rid_t[(unsigned long long)(t + 1u) * n_samples];
    uint32_t w = item_off[t], first = p0; unsigned long long acc = 0;
    for (uint32_t base = p0; base < p1; base += 64u) {
        const uint32_t k = base + lane;
        const uint32_t span = k < p1 ? pairs[k].read_hi - pairs[k].read_lo : 0u;
        const uint32_t n = p1 - base < 64u ? p1 - base : 64u;
        for (uint32_t j = 0; j < n; ++j) {                               // (uniform)
            acc += __shfl(span, (int)j);
            const uint32_t kk = base + j;
            if (acc >= item_intervals || kk + 1u - first >= COV_ITEM_PAIRS || kk + 1u == p1) {
                if (lane == 0) { WorkItem it{}; it.tile = t; it.pair_lo = first; it.pair_hi = kk + 1u; work[w] = it; }
                ++w; first = kk + 1u; acc = 0;
            }
        }
    }
}
__global__ void msnv_fin_pair_flags(const unsigned long long *keys, uint32_t n, uint32_t *flag) {      // (devpack.hip: msnv_pair_flags, the round's copy)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
__global__ void msnv_gather_u32(const uint32_t *src, const unsigned long long *idx, uint32_t n, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}
}  // namespace

int devfin_overhang(msnv_dataset &ds, std::vector<int64_t> &maxend) {
    if (!ds.dp.overhang || !ds.dp.any_overhang_h) return MSNV_OK;   // (the measure kernel of every round said whether a read runs past its contig)
    std::vector<int32_t> oh(ds.names.size());
    HIP_TRY(hipMemcpy(oh.data(), ds.dp.overhang, oh.size() * 4, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < oh.size(); ++c) if (ds.sel[c]) maxend[c] = std::max<int64_t>(maxend[c], oh[c]);
    return MSNV_OK;
}

// d.hdr (allocated, rbase-sized) from the rounds' headers with the positions made linear; needs ds.tile_base
int devfin_headers(msnv_dataset &ds, DeviceCols &d, const std::vector<uint64_t> &rbase) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    DevBuf tb;
    if (int rc = tb.alloc(std::max<size_t>(1, ds.tile_base.size()) * 4)) return rc;
    HIP_TRY(hipMemcpyAsync(tb.p, ds.tile_base.data(), ds.tile_base.size() * 4, hipMemcpyHostToDevice, st));
    for (const DevRound &r : ds.dp.rounds) {
        if (!r.n_pieces) continue;
        hipLaunchKernelGGL(msnv_fin_headers, grid_for(r.n_pieces, 256), dim3(256), 0, st, r.hdr, r.tid, (unsigned long long)r.n_pieces, tb.as<uint32_t>(), d.hdr + rbase[r.first_sample]);
        HIP_TRY(hipGetLastError());
    }
    ds.dp.fin.tile_base = tb.release();                            // (read by kernels that may still be queued: freed with the pack's tables; no wait here)
    return MSNV_OK;
}

namespace {
// One block of device memory handed out piece by piece: take<T>(count) gives the next `count` elements and moves on to the next multiple of
// 256 bytes.  With no block under it the cursor only adds up -- carve_block runs a layout once that way to size the block, allocates, and
// runs it again over the block, so the sum of the sizes and the pointers cannot disagree.
struct Carve {
    uint8_t *base = nullptr; uint64_t at = 0;
    template <typename T> static uint64_t room(uint64_t count) { return (count * sizeof(T) + 255ull) & ~255ull; }
    template <typename T> T *take(uint64_t count) {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += room<T>(count);
        return p;
    }
};
template <typename Lay> int carve_block(void **blk, uint64_t *charge, Lay lay) {
    Carve size; lay(size);
    if (int rc = dev_alloc(blk, size.at, charge)) return rc;
    Carve place{static_cast<uint8_t *>(*blk), 0}; lay(place);
    return MSNV_OK;
}
}  // namespace

// Finalize's pinned result words (devfin.h: FinWords), sized once: whichever of the two stages that queue copies into them comes first
// -- the coverage index launched ahead, the chunk cut -- asks for all of them.
static FinWords fin_words(const msnv_dataset &ds) { return FinWords{reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ds.dp.pin) + ds.dp.pin_cap / 2), ds.samples.size()}; }
static int fin_words_ensure(msnv_dataset &ds, FinWords *w) {
    if (int rc = pin_ensure(ds, FinWords::bytes(ds.samples.size()))) return rc;
    *w = fin_words(ds);
    return MSNV_OK;
}

// Every sample's headers where its round left them (device pointers, one per sample): what msnv_fin_chunks / msnv_fin_merged read.  Built at
// its first use in a finalize and kept (DevPackTables::Fin::sample_hdr) for the later ones, the second cut behind an overflow among them:
// the table holds DevRound::hdr + SampleCols::dev_piece0, and within a fast finalize only the deep-run split (devfin_deep_runs: a round's
// headers through a permutation, into a new buffer) moves either -- in decide_route, before devfin_coverage_launch, which every fast
// finalize passes next and which drops the table of a finalize before it.  devpack_place_columns and devfin_dense move columns, not headers;
// devpack_download_pieces and devpack_add_round do not run inside a fast finalize.
static int sample_hdr_table(msnv_dataset &ds, const ReadHdr *const **out) {
    DevPackTables &T = ds.dp;
    if (!T.fin.sample_hdr) {
        const size_t S = ds.samples.size();
        std::vector<const ReadHdr *> tab(S, nullptr);
        for (size_t s = 0; s < S; ++s) {
            const SampleCols &sc = ds.samples[s];
            if (sc.dev_round >= 0 && (size_t)sc.dev_round < T.rounds.size()) tab[s] = T.rounds[(size_t)sc.dev_round].hdr + sc.dev_piece0;
        }
        void *p = nullptr;
        if (int rc = dev_alloc(&p, std::max<size_t>(1, S) * sizeof(void *), nullptr)) return rc;
        T.fin.keep.push_back(p);
        if (S) HIP_TRY(hipMemcpy(p, tab.data(), S * sizeof(void *), hipMemcpyHostToDevice));
        T.fin.sample_hdr = p;
    }
    *out = static_cast<const ReadHdr *const *>(T.fin.sample_hdr);
    return MSNV_OK;
}

// The narrow pairs' chunks WITHOUT a wait (round 6; round 5 waited for the counts to size the descriptor table and to write the work items'
// ranges): counts -> scan -> fill -> the work items' ranges, all queued; d.chunks (allocated by the caller) has room for `cap` narrow chunks
// behind the `base` chunks of the merged groups, which the host wrote.  cap is the host's bound -- per pair ceil(pieces / CHUNK_READS) + 2: a
// chunk is closed early only where the seq offsets jump by 16 KB, at most once per pair in data the pack laid out --; the true total and an
// overflow flag arrive through the dataset's pinned words (devfin_chunks_result, behind finalize's last wait): an overflow sends finalize
// through this cut once more with the exact count, which is known by then (MSNV_CHUNK_CAP forces it: tests).
int devfin_chunks_launch(msnv_dataset &ds, DeviceCols &d, const std::vector<uint32_t> &narrow_pairs, const std::vector<uint32_t> &item_first, uint32_t base, uint64_t cap) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    DevPackTables::Fin &F = ds.dp.fin;
    const size_t n = narrow_pairs.size(), n_items = item_first.size() - 1;
    FinWords pw;
    if (int rc = fin_words_ensure(ds, &pw)) return rc;
    uint32_t *res = pw.chunks();
    res[0] = 0; res[1] = 0;
    if (!n) return MSNV_OK;
    const ReadHdr *const *s_hdr = nullptr;
    if (int rc = sample_hdr_table(ds, &s_hdr)) return rc;
    void *blk = nullptr;
    uint32_t *list = nullptr, *ifirst = nullptr, *cnt = nullptr, *scan = nullptr, *dres = nullptr;
    if (int rc = carve_block(&blk, nullptr, [&](Carve &c) {
            list = c.take<uint32_t>(n); ifirst = c.take<uint32_t>(n_items + 1); cnt = c.take<uint32_t>(n + 1); scan = c.take<uint32_t>(n + 1); dres = c.take<uint32_t>(2);
        })) return rc;
    F.keep.push_back(blk);
    HIP_TRY(hipMemcpy(list, narrow_pairs.data(), n * 4, hipMemcpyHostToDevice));      // (blocking copies on the null stream: the buffers are fresh, nothing to order against)
    HIP_TRY(hipMemcpy(ifirst, item_first.data(), (n_items + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(cnt + n, 0, 4, st));
    hipLaunchKernelGGL(msnv_fin_chunks<false>, grid_for(n * 64, 256), dim3(256), 0, st, d.pairs, list, (uint32_t)n, s_hdr, (const unsigned long long *)d.s_read_base,
                       (const unsigned long long *)d.s_seq_base, cnt, nullptr, nullptr, nullptr, 0u);
    HIP_TRY(hipGetLastError());
    {
        // (rocPRIM's temporary storage outlives this call: the scan is only queued)
        Prim pr(st);
        const int rc = pr.exclusive(cnt, scan, 0u, n + 1, rocprim::plus<uint32_t>());
        if (pr.own.p) F.keep.push_back(pr.own.release());
        if (rc) return rc;
    }
    hipLaunchKernelGGL(msnv_fin_chunks<true>, grid_for(n * 64, 256), dim3(256), 0, st, d.pairs, list, (uint32_t)n, s_hdr, (const unsigned long long *)d.s_read_base,
                       (const unsigned long long *)d.s_seq_base, nullptr, scan, d.chunks + base, d.hdr4, (uint32_t)std::min<uint64_t>(cap, 0xffffffffull));
    hipLaunchKernelGGL(msnv_fin_work_chunks, grid_for(std::max<size_t>(1, n_items), 256), dim3(256), 0, st, d.work, (uint32_t)n_items, ifirst, scan, (uint32_t)n, base,
                       (uint32_t)std::min<uint64_t>(cap, 0xffffffffull), dres);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(res, dres, 8, hipMemcpyDeviceToHost, st));
    // (an event behind the two words: devfin_chunks_result waits for IT.  Until the coverage tables moved to the device the host's half
    // millisecond of loops over them stood between this launch and the read of the words -- a wait in fact, not in the code)
    if (!F.chunk_event) { hipEvent_t e = nullptr; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); F.chunk_event = e; }
    HIP_TRY(hipEventRecord((hipEvent_t)F.chunk_event, st));
    F.chunk_pending = true;
    return MSNV_OK;
}
// the narrow chunks that were cut, and whether they all found room (waits for the cut's last kernel)
int devfin_chunks_result(msnv_dataset &ds, uint64_t *n_chunks, bool *overflow) {
    DevPackTables::Fin &F = ds.dp.fin;
    if (F.chunk_pending) { F.chunk_pending = false; HIP_TRY(hipEventSynchronize((hipEvent_t)F.chunk_event)); }
    const uint32_t *res = fin_words(ds).chunks();
    *n_chunks = res[0]; *overflow = res[1] != 0;
    return MSNV_OK;
}
int devfin_work_first(msnv_dataset &ds, DeviceCols &d, uint32_t n_items, uint64_t n_room) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    if (n_items) { hipLaunchKernelGGL(msnv_fin_work_first, grid_for(n_items, 256), dim3(256), 0, st, d.work, n_items, d.chunks, (unsigned long long)n_room); HIP_TRY(hipGetLastError()); }
    return MSNV_OK;
}

int devfin_merged_headers(msnv_dataset &ds, DeviceCols &d, const std::vector<DevMergedSrc> &list) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    if (list.empty()) return MSNV_OK;
    const ReadHdr *const *s_hdr = nullptr;
    if (int rc = sample_hdr_table(ds, &s_hdr)) return rc;
    void *l = nullptr;
    if (int rc = dev_alloc(&l, list.size() * sizeof(DevMergedSrc), nullptr)) return rc;
    ds.dp.fin.keep.push_back(l);                                   // (read by a kernel that is only queued: freed with the pack's tables)
    HIP_TRY(hipMemcpy(l, list.data(), list.size() * sizeof(DevMergedSrc), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(msnv_fin_merged, grid_for(list.size(), 64), dim3(64), 0, st, d.pairs, static_cast<const DevMergedSrc *>(l), (uint32_t)list.size(), s_hdr,
                       (const unsigned long long *)d.s_seq_base, d.hdr8m);
    HIP_TRY(hipGetLastError());
    return MSNV_OK;
}

// ------------------------------------------------------------------------------------------ the coverage index
// d.cov_iv (allocated here: kept intervals + 4 idle entries) and, for the host, the kept intervals before every sample (cvbase) and the
// (sample, tile) runs of the intervals in (sample, tile) order.  Three routes over the stages of one CovIndex:
//   launched ahead (round 5; devfin_coverage_launch, as soon as finalize knows the tile layout -- the kernels queue behind whatever the pack
//     left running): prologue, dense_table, dense_runs, table_counts; the small results (per-sample bases, number of runs, the pair tables'
//     counts) land in the pinned words and devfin_coverage only COLLECTS them -- and writes the pair tables there (write_tables) unless the
//     host is to build them.  Dense table form only, and a table of at most 2^24 entries;
//   late dense (MSNV_COV_LATE, or a dense table beyond 2^24 entries; inside devfin_coverage, waiting as it goes): prologue, measure_keep,
//     dense_late (dense_table, a wait for the run count, dense_runs);
//   the sort form (the table would be large beside the interval list): prologue, measure_keep, sort_form.
// Work memory: 12 B per interval (late and sort only) + 24 B per (interval, tile) entry (sort), each group in ONE allocation (hipMalloc /
// hipFree of a dozen multi-gigabyte buffers was most of this step's second at BASELINE configs[2] scale).
static bool cov_dense_form(const msnv_dataset &ds, unsigned long long N) {
    const unsigned long long n_tab = (unsigned long long)ds.samples.size() * ds.n_tiles;
    bool dense_tab = n_tab <= std::max<unsigned long long>(8ull * N, 1ull << 22) && n_tab < 0xfffffff0ull;
    if (const char how = knob::cov_index()) dense_tab = how == 'd' ? n_tab < 0xfffffff0ull : false;
    return dense_tab;
}

namespace {
struct CovIndex {
    msnv_dataset &ds; DeviceCols &d; DevPackTables &T; DevPackTables::Fin &F;
    hipStream_t st; const size_t S;
    Prim pr;
    // ---- the constructor: what both calls know on the host
    std::vector<unsigned long long> iv_start;                      // intervals before every sample, N behind them
    unsigned long long N = 0, n_tab = 0;                           // intervals in all; entries of the dense [sample][tile] table
    const DpContig *ctg = nullptr;
    // ---- prologue (the block is the route's: lay_small)
    uint32_t *tb = nullptr; unsigned long long *ivs = nullptr;     // tile_base and iv_start in HBM
    uint32_t *cvb = nullptr;                                       // kept intervals before every sample [0 .. S]; launched ahead also kept in all [S + 1], runs [S + 2]
    // ---- measure_keep (late and sort)
    DevBuf small, work;
    uint32_t *keep = nullptr, *ntile = nullptr, *kidx = nullptr;   // per interval: kept, tiles it touches, its index among the kept ones
    uint32_t n_keep = 0; std::vector<uint32_t> cvb_h;              // arrive with the next wait for the stream
    // ---- dense_table, dense_runs (the block is the route's: lay_table)
    DevBuf tab, runs_buf;
    uint32_t *lo = nullptr, *hi = nullptr, *flag = nullptr, *rid = nullptr;   // per (sample, tile): first / last + 1 kept interval, "has any", runs before it
    DevCovPair *runs = nullptr;

    CovIndex(msnv_dataset &ds_, DeviceCols &d_)
        : ds(ds_), d(d_), T(ds_.dp), F(ds_.dp.fin), st((hipStream_t)ds_.ctx->stream), S(ds_.samples.size()), pr(st), iv_start(S + 1, 0) {
        for (size_t s = 0; s < S; ++s) iv_start[s + 1] = iv_start[s] + ds.samples[s].n_dev_iv;
        N = iv_start[S];
        n_tab = (unsigned long long)S * ds.n_tiles;
        ctg = static_cast<const DpContig *>(T.contigs);
    }
    void lay_small(Carve &c, size_t n_cvb) { tb = c.take<uint32_t>(std::max<size_t>(1, ds.tile_base.size())); ivs = c.take<unsigned long long>(S + 1); cvb = c.take<uint32_t>(n_cvb); }
    void lay_table(Carve &c) { lo = c.take<uint32_t>(n_tab + 1); hi = c.take<uint32_t>(n_tab + 1); flag = c.take<uint32_t>(n_tab + 1); rid = c.take<uint32_t>(n_tab + 1); }
    // `fn(round, intervals before it)` for every round that has intervals (sample order = round order)
    template <typename Fn> int each_round(Fn fn) {
        unsigned long long o = 0;
        for (const DevRound &r : T.rounds) {
            if (r.n_iv) { fn(r, o); HIP_TRY(hipGetLastError()); }
            o += r.n_iv;
        }
        return MSNV_OK;
    }

    // Takes: tb, ivs laid out.  Leaves: tile_base and iv_start on their way up; the rounds hold the samples' intervals, fewer than 2^32.
    int prologue() {
        if (N > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 qaCompute intervals in one shard");
        unsigned long long o = 0;
        for (const DevRound &r : T.rounds) o += r.n_iv;
        if (o != N) return fail(MSNV_EINVAL, "internal: the rounds hold %llu intervals, the samples %llu", o, N);
        HIP_TRY(hipMemcpyAsync(tb, ds.tile_base.data(), ds.tile_base.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ivs, iv_start.data(), (S + 1) * 8, hipMemcpyHostToDevice, st));
        return MSNV_OK;
    }

    // Takes: the prologue; lo, hi, flag, rid laid out; d.cov_iv allocated; keep_ / kidx_ from measure_keep, or both NULL: every interval is a
    // kept one (the device pack writes no other since round 6) and goes to its own index.  Leaves, queued: d.cov_iv, the table, rid = the runs
    // before every entry and, at [n_tab], their number -- which the caller sends where it is needed before dense_runs.
    int dense_table(const uint32_t *keep_, const uint32_t *kidx_) {
        HIP_TRY(hipMemsetAsync(lo, 0xff, Carve::room<uint32_t>(n_tab + 1), st));
        HIP_TRY(hipMemsetAsync(hi, 0, Carve::room<uint32_t>(n_tab + 1), st));
        if (int rc = each_round([&](const DevRound &r, unsigned long long o) {
                hipLaunchKernelGGL(msnv_fin_cov_emit_dense, grid_for(r.n_iv, 256), dim3(256), 0, st, r.cov_tid, r.cov_beg, r.cov_end, (unsigned long long)r.n_iv, o, ctg, tb, ivs, (uint32_t)S,
                                   keep_, kidx_, ds.n_tiles, d.cov_iv, lo, hi);
            })) return rc;
        hipLaunchKernelGGL(msnv_fin_cov_dense_flags, grid_for(n_tab + 1, 256), dim3(256), 0, st, hi, n_tab, flag);
        HIP_TRY(hipGetLastError());
        return pr.scan32(flag, rid, n_tab + 1, false);
    }
    int dense_runs(DevCovPair *out) {
        hipLaunchKernelGGL(msnv_fin_cov_dense_runs, grid_for(n_tab, 256), dim3(256), 0, st, lo, hi, rid, n_tab, ds.n_tiles, out);
        HIP_TRY(hipGetLastError());
        return MSNV_OK;
    }

    // The route launched ahead.  Takes: ds.tile_base / n_tiles.  Leaves: everything queued, an event behind it, the job's buffers in F (they
    // live until devpack_finish: queued kernels read them), the small results on their way to the pinned words.
    int launch_ahead() {
        FinWords pw;
        if (int rc = fin_words_ensure(ds, &pw)) return rc;
        if (int rc = carve_block(&F.cov_job, nullptr, [&](Carve &c) { lay_small(c, S + 4); lay_table(c); runs = c.take<DevCovPair>(n_tab + 1); })) return rc;
        F.cov_runs = runs;
        if (int rc = prologue()) return rc;
        if (int rc = pr.reserve_scan32(std::max<unsigned long long>(N, n_tab) + 1)) return rc;
        // (every interval of a device-packed round is one the index keeps -- measure_one counts, the emit kernels write, no other: the kept
        // intervals before every sample are the host's iv_start, and nothing is measured or scanned here any more)
        HIP_TRY(hipMemsetAsync(cvb, 0, FinWords::n_kept(S) * 4, st));
        if (int rc = dev_alloc((void **)&d.cov_iv, ((uint64_t)N + 4) * sizeof(Pair32), &d.device_bytes)) return rc;      // (N >= the kept ones: no wait for their count)
        if (int rc = dense_table(nullptr, nullptr)) return rc;
        HIP_TRY(hipMemcpyAsync(cvb + (S + 2), rid + n_tab, 4, hipMemcpyDeviceToDevice, st));
        if (int rc = dense_runs(runs)) return rc;
        HIP_TRY(hipMemcpyAsync(pw.kept(), cvb, FinWords::n_kept(S) * 4, hipMemcpyDeviceToHost, st));      // (pinned: the copy does not wait on the host)
        if (int rc = table_counts(pw)) return rc;
        // an event behind the index's kernels: devfin_coverage waits for IT, not for the stream -- the chunk and header kernels finalize queues
        // behind these run while the host builds the coverage pair tables (round 6)
        if (!F.cov_event) { hipEvent_t e = nullptr; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); F.cov_event = e; }
        HIP_TRY(hipEventRecord((hipEvent_t)F.cov_event, st));
        F.cov_tmp = pr.own.release();                                  // (rocPRIM's work memory: in use until the kernels above have run)
        F.cov_launched = true;
        return MSNV_OK;
    }

    // The pair tables' counts (round 6: the tables themselves are written on the device once the host has allocated them, write_tables).
    // Takes: the dense table queued.  Leaves: F.cov_tables / cov_t (NULL: the host builds the tables -- MSNV_COV_TABLES=host, or no contig, no
    // tile), the four counts and row_start on their way to the pinned words.
    int table_counts(const FinWords &pw) {
        F.cov_tables = nullptr;
        const size_t NC = ds.names.size(), nt = ds.n_tiles;
        const unsigned long long n_sc = (unsigned long long)S * NC;
        if (knob::cov_tables_on_host() || !NC || !nt || ds.tile_contig.size() < nt) return MSNV_OK;
        uint32_t *tcont = nullptr, *flag_t = nullptr, *rid_t = nullptr, *pres = nullptr, *rowid = nullptr, *row_sample = nullptr, *row_contig = nullptr, *n_item = nullptr, *item_off = nullptr,
                 *row_start = nullptr, *counts = nullptr;
        if (int rc = carve_block(&F.cov_tables, nullptr, [&](Carve &c) {
                tcont = c.take<uint32_t>(nt + 1);
                flag_t = c.take<uint32_t>(n_tab + 1); rid_t = c.take<uint32_t>(n_tab + 1);
                pres = c.take<uint32_t>(n_sc + 1); rowid = c.take<uint32_t>(n_sc + 1); row_sample = c.take<uint32_t>(n_sc + 1); row_contig = c.take<uint32_t>(n_sc + 1);
                n_item = c.take<uint32_t>(nt + 2); item_off = c.take<uint32_t>(nt + 2);
                row_start = c.take<uint32_t>(S + 2);
                counts = c.take<uint32_t>(8);                            // [0] pairs [1] rows [2] work items [3] some pair is wide [4] scratch
            })) return rc;
        F.cov_t = DevPackTables::Fin::CovT{tcont, rid_t, rowid, row_sample, row_contig, item_off, lo, hi, ivs};
        HIP_TRY(hipMemcpyAsync(tcont, ds.tile_contig.data(), nt * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(pres, 0, Carve::room<uint32_t>(n_sc + 1), st));
        HIP_TRY(hipMemsetAsync(counts, 0, 32, st));
        const uint32_t item_intervals = knob::cov_item_intervals();
        const uint32_t narrow_max = knob::cov_narrow_max();
        F.cov_item_intervals = item_intervals;
        hipLaunchKernelGGL(msnv_cov_flags_t, grid_for(n_tab + 1, 256), dim3(256), 0, st, hi, (uint32_t)S, ds.n_tiles, tcont, (uint32_t)NC, flag_t, pres);
        HIP_TRY(hipGetLastError());
        if (int rc = pr.scan32(flag_t, rid_t, n_tab + 1, false)) return rc;
        if (int rc = pr.scan32(pres, rowid, n_sc + 1, false)) return rc;
        hipLaunchKernelGGL(msnv_cov_count_items, dim3((unsigned)(nt + 1)), dim3(64), 0, st, lo, hi, (uint32_t)S, ds.n_tiles, item_intervals, narrow_max, n_item, counts + 3);
        HIP_TRY(hipGetLastError());
        if (int rc = pr.scan32(n_item, item_off, nt + 1, false)) return rc;
        hipLaunchKernelGGL(msnv_cov_rows, grid_for(n_sc + 1, 256), dim3(256), 0, st, pres, rowid, (uint32_t)S, (uint32_t)NC, row_sample, row_contig, row_start);
        hipLaunchKernelGGL(msnv_cov_counts, dim3(1), dim3(64), 0, st, rid_t, n_tab, rowid, n_sc, item_off, ds.n_tiles, counts + 3, counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(pw.tables(), counts, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pw.row_start(), row_start, (S + 1) * 4, hipMemcpyDeviceToHost, st));
        return MSNV_OK;
    }

    // Collects the route launched ahead.  Takes: F as launch_ahead left it.  Leaves (behind a wait for the job's event, not for the stream):
    // cvbase, d.n_cov_iv, and either the pair tables written in HBM (F.cov_tables_done) or the runs in cp for the host to build them from.
    // (the job's buffers go back with the pack's tables: a free here would wait for the device)
    int collect(std::vector<uint64_t> &cvbase, std::vector<DevCovPair> &cp) {
        F.cov_launched = false;
        HIP_TRY(hipEventSynchronize((hipEvent_t)F.cov_event));
        const FinWords pw = fin_words(ds);
        for (size_t s = 0; s <= S; ++s) cvbase[s] = iv_start[s];       // (every interval is a kept one)
        const uint32_t n_keep_all = (uint32_t)N, n_runs = pw.n_runs();
        d.n_cov_iv = n_keep_all;
        HIP_TRY(hipMemsetAsync(d.cov_iv + n_keep_all, 0, 4 * sizeof(Pair32), st));          // behind the last interval: what the idle lanes of msnv_coverage_tiles load
        F.cov_tables_done = false;
        if (F.cov_tables && pw.tables()[3] == 0u) {
            if (int rc = write_tables(pw)) return rc;
            fin_trace("    cov: results of the kernels launched ahead, pair tables written there");
            return MSNV_OK;
        }
        cp.resize(n_runs);
        if (n_runs) HIP_TRY(hipMemcpy(cp.data(), F.cov_runs, (size_t)n_runs * sizeof(DevCovPair), hipMemcpyDeviceToHost));      // (a blocking copy on the null stream: the context's stream is still busy, and not waited for)
        fin_trace("    cov: results of the kernels launched ahead");
        return MSNV_OK;
    }
    // The pair tables on the device: their sizes came with the index's counts; the rows' (sample, contig) names come down, nothing else.
    // Takes: the counts in the pinned words, F.cov_t.  Leaves: d.cov_pairs / cov_work (guarded allocations: one each; else one block), ds.cov_row_*.
    int write_tables(const FinWords &pw) {
        const uint32_t n_pairs = pw.tables()[0], n_rows = pw.tables()[1], n_work = pw.tables()[2];
        const size_t NC = ds.names.size();
        const uint64_t b_w = std::max<uint64_t>(16, (uint64_t)(n_work + 1) * sizeof(WorkItem));
        if (knob::guard_alloc()) {
            if (int rc = dev_alloc((void **)&d.cov_pairs, (uint64_t)(n_pairs + 1) * sizeof(TilePair), &d.device_bytes)) return rc;
            if (int rc = dev_alloc((void **)&d.cov_work, b_w, &d.device_bytes)) return rc;
        } else {
            void *blk = nullptr;
            const uint64_t b_p = Carve::room<TilePair>((uint64_t)n_pairs + 1);
            if (int rc = dev_alloc(&blk, b_p + b_w + 256, &d.device_bytes)) return rc;
            d.blocks.emplace_back(blk, b_p + b_w + 256);
            d.cov_pairs = static_cast<TilePair *>(blk);
            d.cov_work = reinterpret_cast<WorkItem *>(static_cast<uint8_t *>(blk) + b_p);
        }
        const DevPackTables::Fin::CovT &C = F.cov_t;
        HIP_TRY(hipMemsetAsync(d.cov_pairs + n_pairs, 0, sizeof(TilePair), st));
        HIP_TRY(hipMemsetAsync(d.cov_work + n_work, 0, sizeof(WorkItem), st));
        if (n_pairs) {
            hipLaunchKernelGGL(msnv_cov_write_pairs, grid_for(n_tab, 256), dim3(256), 0, st, C.lo, C.hi, C.rid_t, C.rowid, C.tcont, C.iv_start, (uint32_t)S, ds.n_tiles, (uint32_t)NC, d.cov_pairs);
            hipLaunchKernelGGL(msnv_cov_write_items, dim3(ds.n_tiles), dim3(64), 0, st, d.cov_pairs, C.rid_t, C.item_off, (uint32_t)S, ds.n_tiles, F.cov_item_intervals, d.cov_work);
            HIP_TRY(hipGetLastError());
        }
        ds.cov_row_sample.assign(n_rows, 0); ds.cov_row_contig.assign(n_rows, 0);
        if (n_rows) {
            HIP_TRY(hipMemcpy(ds.cov_row_sample.data(), C.row_sample, (size_t)n_rows * 4, hipMemcpyDeviceToHost));      // (blocking copies on the null stream: the context's stream is still busy, and not waited for)
            HIP_TRY(hipMemcpy(ds.cov_row_contig.data(), C.row_contig, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
        }
        ds.cov_row_start.assign(pw.row_start(), pw.row_start() + (S + 1));
        d.n_cov_pairs = n_pairs; d.n_cov_work = n_work; d.n_cov_work_wide = 0; d.n_contigs = (uint32_t)NC;
        F.cov_tables_done = true;
        return MSNV_OK;
    }

    // What the late dense route and the sort form share.  Takes: nothing.  Leaves: the prologue done in a block of its own; queued: keep /
    // ntile of every interval where the rounds' intervals lie, kidx = the scan of keep; n_keep and cvb_h, which arrive with the next wait.
    int measure_keep() {
        if (int rc = carve_block(&small.p, nullptr, [&](Carve &c) { lay_small(c, S + 1); })) return rc;
        if (int rc = prologue()) return rc;
        if (int rc = carve_block(&work.p, nullptr, [&](Carve &c) { keep = c.take<uint32_t>(N + 1); ntile = c.take<uint32_t>(N + 1); kidx = c.take<uint32_t>(N + 1); })) return rc;
        if (int rc = each_round([&](const DevRound &r, unsigned long long o) {
                hipLaunchKernelGGL(msnv_fin_cov_measure, grid_for(r.n_iv, 256), dim3(256), 0, st, r.cov_tid, r.cov_beg, r.cov_end, (unsigned long long)r.n_iv, ctg, tb, keep + o, ntile + o);
            })) return rc;
        HIP_TRY(hipMemsetAsync(keep + N, 0, 4, st));
        HIP_TRY(hipMemsetAsync(ntile + N, 0, 4, st));
        fin_trace("    cov: allocs + measure launched");
        if (int rc = pr.scan32(keep, kidx, N + 1, false)) return rc;
        HIP_TRY(hipMemcpyAsync(&n_keep, kidx + N, 4, hipMemcpyDeviceToHost, st));
        hipLaunchKernelGGL(msnv_gather_u32, grid_for(S + 1, 64), dim3(64), 0, st, kidx, ivs, (uint32_t)(S + 1), cvb);
        HIP_TRY(hipGetLastError());
        cvb_h.resize(S + 1);
        HIP_TRY(hipMemcpyAsync(cvb_h.data(), cvb, (S + 1) * 4, hipMemcpyDeviceToHost, st));
        return MSNV_OK;
    }

    // The dense table inside devfin_coverage (MSNV_COV_LATE; a table beyond 2^24 entries; MSNV_COV_INDEX=dense).  Takes: measure_keep.
    // Leaves, behind two waits for the stream: d.cov_iv / n_cov_iv, cvbase, the runs in cp.
    int dense_late(std::vector<uint64_t> &cvbase, std::vector<DevCovPair> &cp) {
        d.n_cov_iv = 0;
        if (int rc = dev_alloc((void **)&d.cov_iv, ((uint64_t)N + 4) * sizeof(Pair32), &d.device_bytes)) return rc;      // (N >= the kept ones: no wait for their count)
        if (int rc = carve_block(&tab.p, nullptr, [&](Carve &c) { lay_table(c); })) return rc;
        if (int rc = dense_table(keep, kidx)) return rc;
        uint32_t n_runs = 0;
        HIP_TRY(hipMemcpyAsync(&n_runs, rid + n_tab, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));                               // (n_keep and the per-sample bases arrive with it)
        for (size_t s = 0; s <= S; ++s) cvbase[s] = cvb_h[s];
        d.n_cov_iv = n_keep;
        HIP_TRY(hipMemsetAsync(d.cov_iv + n_keep, 0, 4 * sizeof(Pair32), st));              // behind the last interval: what the idle lanes of msnv_coverage_tiles load
        if (int rc = runs_buf.alloc(std::max<uint64_t>(1, n_runs) * sizeof(DevCovPair))) return rc;
        if (int rc = dense_runs(runs_buf.as<DevCovPair>())) return rc;
        cp.resize(n_runs);
        if (n_runs) HIP_TRY(hipMemcpyAsync(cp.data(), runs_buf.p, (size_t)n_runs * sizeof(DevCovPair), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        fin_trace("    cov: dense table, runs (sync)");
        return MSNV_OK;
    }

    // The sort form: an entry (sample, tile, index) per interval and tile it touches, sorted; a run = the entries of one (sample, tile).
    // Takes: measure_keep.  Leaves, behind its waits for the stream: d.cov_iv / n_cov_iv, cvbase, the runs in cp.
    int sort_form(std::vector<uint64_t> &cvbase, std::vector<DevCovPair> &cp) {
        // entry slots: exclusive scan of the tile counts, in place of `keep` (no longer needed once kidx exists)
        unsigned long long n_ent64 = 0;
        {
            DevBuf tot;
            if (int rc = tot.alloc(16)) return rc;
            // (a 64-bit total first: the 32-bit scan below must not wrap)
            size_t need = 0;
            HIP_TRY(rocprim::reduce(nullptr, need, ntile, tot.as<unsigned long long>(), 0ull, (size_t)N, rocprim::plus<unsigned long long>(), st));
            if (int rc = pr.room(need)) return rc;
            HIP_TRY(rocprim::reduce(pr.buf, need, ntile, tot.as<unsigned long long>(), 0ull, (size_t)N, rocprim::plus<unsigned long long>(), st));
            HIP_TRY(hipMemcpyAsync(&n_ent64, tot.p, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        fin_trace("    cov: scans + reduce (sync)");
        if (n_ent64 > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 (interval, tile) entries in one shard");
        const uint32_t n_ent = (uint32_t)n_ent64;
        uint32_t *ebase = keep;
        if (int rc = pr.scan32(ntile, ebase, N + 1, false)) return rc;
        for (size_t s = 0; s <= S; ++s) cvbase[s] = cvb_h[s];
        d.n_cov_iv = n_keep;
        if (int rc = dev_alloc((void **)&d.cov_iv, ((uint64_t)n_keep + 4) * sizeof(Pair32), &d.device_bytes)) return rc;
        HIP_TRY(hipMemsetAsync(d.cov_iv + n_keep, 0, 4 * sizeof(Pair32), st));                  // behind the last interval: what the idle lanes of msnv_coverage_tiles load
        DevBuf ent;
        unsigned long long *ekey = nullptr, *skey = nullptr; uint32_t *eval = nullptr, *sval = nullptr;
        if (int rc = carve_block(&ent.p, nullptr, [&](Carve &c) {
                ekey = c.take<unsigned long long>((uint64_t)n_ent + 1); skey = c.take<unsigned long long>((uint64_t)n_ent + 1); eval = c.take<uint32_t>((uint64_t)n_ent + 1); sval = c.take<uint32_t>((uint64_t)n_ent + 1);
            })) return rc;
        if (int rc = each_round([&](const DevRound &r, unsigned long long o) {
                hipLaunchKernelGGL(msnv_fin_cov_emit, grid_for(r.n_iv, 256), dim3(256), 0, st, r.cov_tid, r.cov_beg, r.cov_end, (unsigned long long)r.n_iv, o, ctg, tb, ivs, (uint32_t)S,
                                   ntile + o, kidx, ebase + o, d.cov_iv, ekey, eval);
            })) return rc;
        fin_trace("    cov: allocs + emit launched");
        if (n_ent) {
            if (int rc = pr.sort64(ekey, skey, eval, sval, n_ent, 32u + std::max(1u, bit_width_u64(S)))) return rc;
            // runs of equal (sample, tile): flags and their scan in the unsorted arrays' memory (dead behind the sort)
            uint32_t *eflag = eval, *erid = reinterpret_cast<uint32_t *>(ekey);
            hipLaunchKernelGGL(msnv_fin_pair_flags, grid_for(n_ent, 256), dim3(256), 0, st, skey, n_ent, eflag);
            HIP_TRY(hipGetLastError());
            if (int rc = pr.scan32(eflag, erid, n_ent, true)) return rc;
            uint32_t n_runs = 0;
            HIP_TRY(hipMemcpyAsync(&n_runs, erid + (n_ent - 1), 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = runs_buf.alloc((uint64_t)n_runs * sizeof(DevCovPair))) return rc;
            hipLaunchKernelGGL(msnv_fin_cov_runs, grid_for(n_ent, 256), dim3(256), 0, st, skey, sval, eflag, erid, (unsigned long long)n_ent, runs_buf.as<DevCovPair>());
            HIP_TRY(hipGetLastError());
            cp.resize(n_runs);
            HIP_TRY(hipMemcpyAsync(cp.data(), runs_buf.p, (size_t)n_runs * sizeof(DevCovPair), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            fin_trace("    cov: sort + runs (sync)");
        }
        HIP_TRY(hipStreamSynchronize(st));
        return MSNV_OK;
    }
};
}  // namespace

// The coverage index's kernels ahead of their results.  Nothing is launched -- devfin_coverage then runs the index itself, waiting as it
// goes -- when the intervals do not fit 32 bits (its error), the sort form is due, the dense table is beyond 2^24 entries, or MSNV_COV_LATE.
int devfin_coverage_launch(msnv_dataset &ds, DeviceCols &d) {
    ds.dp.fin.sample_hdr = nullptr;                                // (a fast finalize begins here, behind the deep-run split: sample_hdr_table)
    CovIndex C(ds, d);
    if (C.N > 0xfffffff0ull || !cov_dense_form(ds, C.N) || C.n_tab > (1ull << 24) || knob::cov_late()) return MSNV_OK;
    return C.launch_ahead();
}

int devfin_coverage(msnv_dataset &ds, DeviceCols &d, std::vector<uint64_t> &cvbase, std::vector<DevCovPair> &cp) {
    CovIndex C(ds, d);
    cvbase.assign(C.S + 1, 0); cp.clear();
    C.F.cov_tables_done = false;
    if (C.F.cov_launched) return C.collect(cvbase, cp);
    if (int rc = C.measure_keep()) return rc;
    // the (sample, tile) runs: a dense table of minima / maxima when it is small beside the interval list (MSNV_COV_INDEX=sort|dense forces one)
    return cov_dense_form(ds, C.N) ? C.dense_late(cvbase, cp) : C.sort_form(cvbase, cp);
}

// ------------------------------------------------------------------------------------------ deep runs (finalize.cpp: split_deep_runs)
namespace {
__device__ __forceinline__ int wave_inclusive_scan_int(int v) {
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(v, o); if ((int)(threadIdx.x & 63u) >= o) v += y; }
    return v;
}
constexpr uint32_t DEEP_G_CAP = 512;                              // groups a run may be dealt into (depth cap 65535 / group depth 128)
struct DevDeepRun { unsigned long long piece0; uint32_t n, pad; };   // pieces [piece0, piece0 + n) of a ROUND's header array
struct DevDeepOut { uint32_t G, exact; };                            // G = 1: not split, `exact` is the run's true depth; G > 1: dealt into G groups (their depths in gmax); G = 0: too many groups
// largest per-position depth of the pieces g, g + G, g + 2G, ... of the run (one workgroup of 256, a difference array of the tile in LDS)
__device__ uint32_t deep_sweep(const ReadHdr *h, const uint32_t n, const uint32_t G, const uint32_t g, int *diff, int *wsum) {
    const int tid = threadIdx.x;
    for (int i = tid; i < (int)TILE + 8; i += 256) diff[i] = 0;
    __syncthreads();
    for (uint32_t j = g + G * (uint32_t)tid; j < n; j += G * 256u) {
        const ReadHdr x = h[j];
        const uint32_t s0 = x.gpos % TILE;
        atomicAdd(&diff[s0], 1); atomicAdd(&diff[s0 + x.cig], -1);
    }
    __syncthreads();
    int v[8], sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = diff[8 * tid + k]; sum += v[k]; }
    const int incl = wave_inclusive_scan_int(sum);
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) base += wsum[w];
    int m = 0, cur = base;
#pragma unroll
    for (int k = 0; k < 8; ++k) { cur += v[k]; m = cur > m ? cur : m; }
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_down(m, o); m = y > m ? y : m; }
    __syncthreads();
    if ((tid & 63) == 0) wsum[4 + (tid >> 6)] = m;
    __syncthreads();
    const int r = max(max(wsum[4], wsum[5]), max(wsum[6], wsum[7]));
    __syncthreads();
    return (uint32_t)r;
}
__global__ __launch_bounds__(256) void msnv_fin_deep_sweep(const ReadHdr *hdr, const DevDeepRun *runs, uint32_t split_at, uint32_t group_depth, DevDeepOut *outs, uint32_t *gmax) {
    __shared__ int diff[TILE + 8];
    __shared__ int wsum[8];
    const DevDeepRun r = runs[blockIdx.x];
    const ReadHdr *h = hdr + r.piece0;
    uint32_t *gm = gmax + (size_t)blockIdx.x * DEEP_G_CAP;
    const uint32_t exact = deep_sweep(h, r.n, 1u, 0u, diff, wsum);
    if (exact < split_at) { if (threadIdx.x == 0) outs[blockIdx.x] = DevDeepOut{1u, exact}; return; }
    uint32_t G = exact / group_depth + 1u;
    for (;; ++G) {
        if (G > DEEP_G_CAP) { if (threadIdx.x == 0) outs[blockIdx.x] = DevDeepOut{0u, exact}; return; }
        uint32_t worst = 0;
        for (uint32_t g = 0; g < G; ++g) { const uint32_t d = deep_sweep(h, r.n, G, g, diff, wsum); if (threadIdx.x == 0) gm[g] = d; worst = d > worst ? d : worst; }
        if (worst < NARROW_MAX_DEPTH) break;
    }
    if (threadIdx.x == 0) outs[blockIdx.x] = DevDeepOut{G, exact};
}
// where the piece that ends up at position j of a split run comes from: groups one after the other, a group's pieces in their old order
struct DevDeepPerm { unsigned long long piece0; uint32_t n, G; };
__global__ void msnv_fin_deep_perm(const DevDeepPerm *runs, uint32_t *src) {
    const DevDeepPerm r = runs[blockIdx.x];
    const uint32_t q = r.n / r.G, rem = r.n % r.G;
    for (uint32_t k = threadIdx.x; k < r.n; k += blockDim.x) {
        const uint32_t g = k % r.G, newpos = g * q + (g < rem ? g : rem) + k / r.G;
        src[r.piece0 + newpos] = (uint32_t)(r.piece0 + k);
    }
}
__global__ void msnv_iota(uint32_t *a, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (uint32_t)i;
}
__global__ void msnv_fin_stored(const ReadHdr *hdr, unsigned long long n, uint32_t *out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) out[i] = i < n ? stored_bytes(hdr[i].cig) : 0u;
}
// a sample's columns re-laid in header order: 4 lanes per piece, 32 stored nibbles per lane, from the old offsets to the new
__global__ __launch_bounds__(256) void msnv_fin_relayout(ReadHdr *hdr, unsigned long long n_pieces, const uint32_t *new_off, const uint8_t *old_seq, const uint8_t *old_qual,
                                                         uint8_t *new_seq, uint8_t *new_qual) {
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long pc = gt >> 2; const uint32_t sub = (uint32_t)gt & 3u;
    ReadHdr h{}; uint32_t sb = 0, noff = 0;
    if (pc < n_pieces) { h = hdr[pc]; sb = stored_bytes(h.cig); noff = new_off[pc]; }
    const uint32_t st = 2u * sb > 32u * sub ? (2u * sb - 32u * sub < 32u ? 2u * sb - 32u * sub : 32u) : 0u;
    uint64_t o0 = 0, o1 = 0; uint32_t bits = 0;
    if (st) {
        const uint8_t *sp = old_seq + h.seqoff + 16u * sub;
        o0 = ld64(sp); o1 = ld64(sp + 8);
        const unsigned long long b = 2ull * h.seqoff + 32u * sub;
        bits = (uint32_t)(ld64(old_qual + (b >> 3)) >> (uint32_t)(b & 7ull));
    }
    const uint32_t prev_last = __shfl_up(bits >> 28, 1);
    if (st) put_piece_lane(new_seq, new_qual, noff, sub, sb, st, o0, o1, bits, prev_last);
    if (st && sub == 0) hdr[pc].seqoff = noff;                     // (every lane of the piece has read its header by now: the loads sit above the shuffle)
}
}  // namespace

int devfin_deep_runs(msnv_dataset &ds, uint32_t split_at, uint32_t group_depth, bool *fallback) {
    *fallback = false;
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    DevPackTables &T = ds.dp;
    const size_t S = ds.samples.size();
    // ---- the runs whose bound reaches split_at, round by round
    struct Ref { size_t sample, pair; };
    std::vector<std::vector<DevDeepRun>> runs(T.rounds.size());
    std::vector<std::vector<Ref>> refs(T.rounds.size());
    for (size_t s = 0; s < S; ++s) {
        const SampleCols &sc = ds.samples[s];
        for (size_t k = 0; k < sc.dev_pairs.size(); ++k) if (sc.dev_pairs[k].maxd >= split_at) {
            runs[(size_t)sc.dev_round].push_back(DevDeepRun{sc.dev_piece0 + sc.dev_pairs[k].lo, sc.dev_pairs[k].hi - sc.dev_pairs[k].lo, 0u});
            refs[(size_t)sc.dev_round].push_back(Ref{s, k});
        }
    }
    std::vector<uint8_t> split_sample(S, 0);
    std::vector<std::vector<DevDeepPerm>> perms(T.rounds.size());
    struct NewPairs { size_t pair; uint32_t G; std::vector<uint32_t> gmax; };
    std::vector<std::vector<NewPairs>> edits(S);
    for (size_t r = 0; r < T.rounds.size(); ++r) {
        const size_t n = runs[r].size();
        if (!n) continue;
        DevBuf d_runs, d_outs, d_gmax;
        if (int rc = d_runs.alloc(n * sizeof(DevDeepRun))) return rc;
        if (int rc = d_outs.alloc(n * sizeof(DevDeepOut))) return rc;
        if (int rc = d_gmax.alloc(n * DEEP_G_CAP * 4)) return rc;
        HIP_TRY(hipMemcpyAsync(d_runs.p, runs[r].data(), n * sizeof(DevDeepRun), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(msnv_fin_deep_sweep, dim3((unsigned)n), dim3(256), 0, st, T.rounds[r].hdr, d_runs.as<DevDeepRun>(), split_at, group_depth, d_outs.as<DevDeepOut>(), d_gmax.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        std::vector<DevDeepOut> outs(n);
        std::vector<uint32_t> gmax(n * DEEP_G_CAP);
        HIP_TRY(hipMemcpyAsync(outs.data(), d_outs.p, n * sizeof(DevDeepOut), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(gmax.data(), d_gmax.p, n * DEEP_G_CAP * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < n; ++i) {
            const Ref ref = refs[r][i];
            SampleCols &sc = ds.samples[ref.sample];
            if (outs[i].G == 0u) { *fallback = true; return MSNV_OK; }
            if (outs[i].G == 1u) { sc.dev_pairs[ref.pair].maxd = outs[i].exact; continue; }      // the start-time bound was pessimistic
            split_sample[ref.sample] = 1;
            ++T.n_deep_runs_split;
            perms[r].push_back(DevDeepPerm{runs[r][i].piece0, runs[r][i].n, outs[i].G});
            edits[ref.sample].push_back(NewPairs{ref.pair, outs[i].G, std::vector<uint32_t>(gmax.begin() + i * DEEP_G_CAP, gmax.begin() + i * DEEP_G_CAP + outs[i].G)});
        }
    }
    // ---- the pair lists of the samples with split runs: a run of n pieces in G groups becomes G pairs (group g: the pieces g, g + G, ...)
    for (size_t s = 0; s < S; ++s) {
        if (edits[s].empty()) continue;
        SampleCols &sc = ds.samples[s];
        std::vector<DevPair> np;
        size_t e = 0;
        for (size_t k = 0; k < sc.dev_pairs.size(); ++k) {
            const DevPair p = sc.dev_pairs[k];
            if (e < edits[s].size() && edits[s][e].pair == k) {
                const uint32_t n = p.hi - p.lo, G = edits[s][e].G, q = n / G, rem = n % G;
                uint32_t lo = p.lo;
                for (uint32_t g = 0; g < G; ++g) { const uint32_t cnt = q + (g < rem ? 1u : 0u); if (cnt) np.push_back(DevPair{p.tid, p.tile, lo, lo + cnt, edits[s][e].gmax[g], 1u + g}); lo += cnt; }
                ++e;
            } else np.push_back(p);
        }
        sc.dev_pairs.swap(np);
    }
    // ---- headers of the split runs group by group, then the columns of their samples in header order
    for (size_t r = 0; r < T.rounds.size(); ++r) {
        if (perms[r].empty()) continue;
        DevRound &R = T.rounds[r];
        DevBuf d_perm, d_src;
        if (int rc = d_perm.alloc(perms[r].size() * sizeof(DevDeepPerm))) return rc;
        if (int rc = d_src.alloc((R.n_pieces + 1) * 4)) return rc;
        HIP_TRY(hipMemcpyAsync(d_perm.p, perms[r].data(), perms[r].size() * sizeof(DevDeepPerm), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(msnv_iota, grid_for(R.n_pieces, 256), dim3(256), 0, st, d_src.as<uint32_t>(), (unsigned long long)R.n_pieces);
        hipLaunchKernelGGL(msnv_fin_deep_perm, dim3((unsigned)perms[r].size()), dim3(256), 0, st, d_perm.as<DevDeepPerm>(), d_src.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        // the round's headers through the permutation, into a buffer of their own (the intervals stay where they are)
        const uint64_t b_hdr = R.n_pieces * sizeof(ReadHdr), b_4 = ((R.n_pieces * 4) + 15) & ~15ull, b_2 = ((R.n_pieces * 2) + 15) & ~15ull;
        void *nb = nullptr;
        if (int rc = dev_alloc(&nb, b_hdr + 2 * b_4 + b_2 + 64, nullptr)) return rc;
        uint8_t *q = static_cast<uint8_t *>(nb);
        ReadHdr *h2 = reinterpret_cast<ReadHdr *>(q); q += b_hdr;
        int32_t *t2 = reinterpret_cast<int32_t *>(q); q += b_4;
        int32_t *e2 = reinterpret_cast<int32_t *>(q); q += b_4;
        uint16_t *d2 = reinterpret_cast<uint16_t *>(q);
        if (int rc = devpack_gather_pieces(st, d_src.as<uint32_t>(), R, h2, t2, e2, d2)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        T.round_bufs.push_back(R.buf);                             // (the old buffer still holds the round's intervals; freed with the columns)
        R.buf = nb; R.hdr = h2; R.tid = t2; R.end = e2; R.depth = d2;
    }
    Prim pr(st);
    for (size_t s = 0; s < S; ++s) {
        if (!split_sample[s]) continue;
        SampleCols &sc = ds.samples[s];
        DevRound &R = T.rounds[(size_t)sc.dev_round];
        ReadHdr *h = R.hdr + sc.dev_piece0;
        const unsigned long long n = sc.n_dev_pieces;
        DevBuf d_st, d_off;
        if (int rc = d_st.alloc((n + 1) * 4)) return rc;
        if (int rc = d_off.alloc((n + 1) * 4)) return rc;
        hipLaunchKernelGGL(msnv_fin_stored, grid_for(n + 1, 256), dim3(256), 0, st, h, n, d_st.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        if (int rc = pr.scan32(d_st.as<uint32_t>(), d_off.as<uint32_t>(), n + 1, false)) return rc;
        const uint64_t seq_bytes = (sc.d_seq_bytes + 15) & ~15ull, qual_bytes = seq_bytes / 4;
        void *nb = nullptr;
        if (int rc = dev_alloc(&nb, seq_bytes + qual_bytes + 64, nullptr)) return rc;
        T.round_bufs.push_back(nb);
        uint8_t *nseq = static_cast<uint8_t *>(nb), *nqual = nseq + seq_bytes;
        HIP_TRY(hipMemsetAsync(nseq, 0xff, seq_bytes, st));
        HIP_TRY(hipMemsetAsync(nqual, 0, qual_bytes + 64, st));
        hipLaunchKernelGGL(msnv_fin_relayout, grid_for(n * 4, 256), dim3(256), 0, st, h, n, d_off.as<uint32_t>(), sc.d_seq, sc.d_qual, nseq, nqual);
        HIP_TRY(hipGetLastError());
        // tail: 32 bytes of N (the memset) and their flags, by the round's own kernel; waits for the stream
        if (int rc = devpack_emit_tail(ds, nseq, nqual, sc.d_seq_bytes - 32)) return rc;
        sc.d_seq = nseq; sc.d_qual = nqual;
    }
    return MSNV_OK;
}

// ------------------------------------------------------------------------------------------ dense block streams (short reads)
// finalize.cpp: relayout_dense as kernels.  A run's stream is cut into blocks of 32 bases: a piece starts on an even base, opens a fresh block
// when the block it would start in already holds a second segment or when it would end inside that block.  One thread walks one run (the
// rule is sequential inside a run): first to count the run's blocks, then -- block bases known -- to write descriptors and the pieces' new
// offsets; the bases and flags move with four lanes per piece.
namespace {
struct DevDenseRun { unsigned long long piece0; uint32_t n, blk0, seq0, pad; };        // blk0: index into the round's block array; seq0: byte offset of the run in its sample's seq column
template <bool WRITE>
__device__ __forceinline__ uint32_t dense_walk(const ReadHdr *h, uint32_t n, uint32_t seq0, uint32_t *blk, uint32_t *new_off) {
    uint32_t cursor = 0, nblk = 0, lastw = BLK_EMPTY;                                   // lastw: descriptor of block nblk - 1, not yet written
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t len = h[k].cig, P = h[k].gpos % TILE;
        cursor = (cursor + 1u) & ~1u;
        uint32_t o = cursor & 31u;
        if (o != 0u) {                                                                  // (then the block holding `cursor` is block nblk - 1)
            const bool has_b = ((lastw >> 17) & 0xfffu) != BLK_NO_B;
            if (has_b || len < 32u - o) { cursor = ((cursor >> 5) + 1u) << 5; o = 0u; }
        }
        if (WRITE) new_off[k] = seq0 + (cursor >> 1);
        uint32_t done = 0;
        if (o != 0u) {                                                                  // the head of the piece = segment B of the open block
            lastw = (lastw & ~(0xfffu << 17)) | ((P - o + 32u) << 17);
            done = 32u - o;
            if (done == len) lastw |= BLK_END_B;
        }
        bool first = o == 0u;
        while (done < len) {
            const uint32_t na = len - done < 32u ? len - done : 32u;
            if (WRITE && nblk) blk[nblk - 1u] = lastw;
            ++nblk;
            lastw = BLK_EMPTY | (P + done) | na << 11 | (first ? BLK_START_A : 0u) | (done + na == len ? BLK_END_A : 0u);
            first = false; done += na;
        }
        cursor += len;
    }
    if (WRITE && nblk) blk[nblk - 1u] = lastw;
    return nblk;
}
__global__ void msnv_fin_dense_count(const ReadHdr *hdr, const DevDenseRun *runs, uint32_t n_runs, uint32_t *nblk) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    nblk[r] = dense_walk<false>(hdr + runs[r].piece0, runs[r].n, 0u, nullptr, nullptr);
}
__global__ void msnv_fin_dense_place(const ReadHdr *hdr, const DevDenseRun *runs, uint32_t n_runs, uint32_t *blk, uint32_t *new_off) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const DevDenseRun R = runs[r];
    dense_walk<true>(hdr + R.piece0, R.n, R.seq0, blk + R.blk0, new_off + R.piece0);
}
// bits [b0, b0 + n) of a flag column := the n low bits of v (n <= 32).  The column was filled with `ones` everywhere; whole bytes are stored,
// the bytes shared with a neighbour get ONE atomic (clear what must be 0, or set what must be 1).
__device__ __forceinline__ void and_byte(uint8_t *p, uint32_t v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t sh = 8u * (uint32_t)(a & 3u);
    atomicAnd(reinterpret_cast<uint32_t *>(a & ~(uintptr_t)3), ~(0xffu << sh) | v << sh);
}
__device__ __forceinline__ void put_flag_bits(uint8_t *col, unsigned long long b0, uint32_t n, uint32_t v, bool ones) {
    uint8_t *p = col + (b0 >> 3);
    const uint32_t sh = (uint32_t)(b0 & 7ull);
    const uint64_t m = (n < 32u ? (1ull << n) - 1ull : 0xffffffffull) << sh, w = ((uint64_t)v << sh) & m;
    const uint32_t nbytes = (sh + n + 7u) >> 3;
    for (uint32_t k = 0; k < nbytes; ++k) {
        const uint32_t mb = (uint32_t)(m >> (8u * k)) & 0xffu, wb = (uint32_t)(w >> (8u * k)) & 0xffu;
        if (mb == 0xffu) p[k] = (uint8_t)wb;
        else if (ones) and_byte(p + k, (~mb | wb) & 0xffu);
        else if (wb) or_byte(p + k, wb);
    }
}
// the pieces of one sample into its dense columns: 4 lanes per piece, 32 bases per lane, nothing but the real bases moves
__global__ __launch_bounds__(256) void msnv_fin_dense_copy(ReadHdr *hdr, unsigned long long n_pieces, const uint32_t *new_off, const uint8_t *old_seq, const uint8_t *old_qual,
                                                           uint8_t *new_seq, uint8_t *new_qual, uint32_t ones) {
    const unsigned long long gt = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long pc = gt >> 2; const uint32_t sub = (uint32_t)gt & 3u, j0 = 32u * sub;
    ReadHdr h{}; uint32_t noff = 0;
    if (pc < n_pieces) { h = hdr[pc]; noff = new_off[pc]; }
    const uint32_t have = h.cig > j0 ? (h.cig - j0 < 32u ? h.cig - j0 : 32u) : 0u;
    if (have) {
        const uint8_t *sp = old_seq + h.seqoff + 16u * sub;
        uint64_t o0 = ld64(sp), o1 = ld64(sp + 8);
        if (have & 1u) { if (have < 16u) o0 |= 0xfull << (4u * have); else o1 |= 0xfull << (4u * (have - 16u)); }      // the pad nibble of an odd piece reads as N
        const uint32_t nb = (have + 1u) >> 1;
        uint8_t *dp = new_seq + noff + 16u * sub;
        store_bytes(dp, o0, nb < 8u ? nb : 8u);
        if (nb > 8u) store_bytes(dp + 8, o1, nb - 8u);
        const unsigned long long b = 2ull * h.seqoff + j0;
        const uint32_t bits = (uint32_t)(ld64(old_qual + (b >> 3)) >> (uint32_t)(b & 7ull));
        put_flag_bits(new_qual, 2ull * noff + j0, have, bits, ones != 0u);
    }
    if (have && sub == 0) hdr[pc].seqoff = noff;                   // (the four lanes of a piece sit in one wavefront: all of them have read the header)
}
}  // namespace

int devfin_dense(msnv_dataset &ds) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    DevPackTables &T = ds.dp;
    const size_t S = ds.samples.size();
    const msnv_params &MP = ds.params;
    const bool ones = std::min(std::max(MP.min_baseq, -127), 127) > 0 || MP.min_baseq > 127;      // what a padding byte's flag is (finalize.cpp: pack_lowq of a 0 byte)
    for (size_t r = 0; r < T.rounds.size(); ++r) {
        DevRound &R = T.rounds[r];
        std::vector<DevDenseRun> runs;
        std::vector<size_t> s_of;                                    // samples of this round, in order
        for (size_t s = 0; s < S; ++s) if (ds.samples[s].dev_index && (size_t)ds.samples[s].dev_round == r) {
            s_of.push_back(s);
            for (const DevPair &p : ds.samples[s].dev_pairs) runs.push_back(DevDenseRun{ds.samples[s].dev_piece0 + p.lo, p.hi - p.lo, 0u, 0u, 0u});
        }
        if (s_of.empty()) continue;
        const size_t n = runs.size();
        std::vector<uint32_t> nblk(n, 0);
        DevBuf d_runs, d_nblk, d_off;
        if (n) {
            if (int rc = d_runs.alloc(n * sizeof(DevDenseRun))) return rc;
            if (int rc = d_nblk.alloc(n * 4)) return rc;
            HIP_TRY(hipMemcpyAsync(d_runs.p, runs.data(), n * sizeof(DevDenseRun), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(msnv_fin_dense_count, grid_for(n, 64), dim3(64), 0, st, R.hdr, d_runs.as<DevDenseRun>(), (uint32_t)n, d_nblk.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(nblk.data(), d_nblk.p, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        // block bases: per sample (run_* as relayout_dense leaves them), and where the sample's blocks and columns sit in the round's buffers
        std::vector<uint64_t> blk_at(s_of.size() + 1, 0), col_at(s_of.size() + 1, 0);
        size_t k = 0;
        for (size_t i = 0; i < s_of.size(); ++i) {
            SampleCols &sc = ds.samples[s_of[i]];
            sc.run_blk_lo.clear(); sc.run_nblk.clear(); sc.run_seq0.clear();
            uint64_t b = 0;
            for (size_t j = 0; j < sc.dev_pairs.size(); ++j, ++k) {
                if (b + nblk[k] > 0x07ffffffull) return fail(MSNV_EDOMAIN, "a sample's dense block stream exceeds 2^27 blocks");
                runs[k].blk0 = (uint32_t)(blk_at[i] + b); runs[k].seq0 = (uint32_t)(16u * b);
                sc.run_blk_lo.push_back((uint32_t)b); sc.run_nblk.push_back(nblk[k]); sc.run_seq0.push_back((uint32_t)(16u * b));
                b += nblk[k];
            }
            if (blk_at[i] + b > 0xfffffff0ull) return fail(MSNV_EDOMAIN, "more than 2^32 dense blocks in one round");
            blk_at[i + 1] = blk_at[i] + b;
            const uint64_t seq_bytes = 16ull * b + 32ull;            // + the tail padding
            col_at[i + 1] = col_at[i] + ((seq_bytes + seq_bytes / 4 + 64ull + 15ull) & ~15ull);
        }
        void *colbuf = nullptr, *blkbuf = nullptr;
        if (int rc = dev_alloc(&colbuf, col_at.back() + 64, nullptr)) return rc;
        T.round_bufs.push_back(colbuf);
        if (int rc = dev_alloc(&blkbuf, (blk_at.back() + 1) * 4, nullptr)) return rc;
        T.round_bufs.push_back(blkbuf);
        if (n) {
            if (int rc = d_off.alloc((R.n_pieces + 1) * 4)) return rc;
            HIP_TRY(hipMemcpyAsync(d_runs.p, runs.data(), n * sizeof(DevDenseRun), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(msnv_fin_dense_place, grid_for(n, 64), dim3(64), 0, st, R.hdr, d_runs.as<DevDenseRun>(), (uint32_t)n, static_cast<uint32_t *>(blkbuf), d_off.as<uint32_t>());
            HIP_TRY(hipGetLastError());
        }
        for (size_t i = 0; i < s_of.size(); ++i) {
            SampleCols &sc = ds.samples[s_of[i]];
            const uint64_t seq_bytes = 16ull * (blk_at[i + 1] - blk_at[i]) + 32ull;
            uint8_t *nseq = static_cast<uint8_t *>(colbuf) + col_at[i], *nqual = nseq + seq_bytes;
            HIP_TRY(hipMemsetAsync(nseq, 0xff, seq_bytes, st));
            HIP_TRY(hipMemsetAsync(nqual, ones ? 0xff : 0, seq_bytes / 4, st));
            if (sc.n_dev_pieces) {
                hipLaunchKernelGGL(msnv_fin_dense_copy, grid_for(sc.n_dev_pieces * 4, 256), dim3(256), 0, st, R.hdr + sc.dev_piece0, (unsigned long long)sc.n_dev_pieces,
                                   d_off.as<uint32_t>() + sc.dev_piece0, sc.d_seq, sc.d_qual, nseq, nqual, ones ? 1u : 0u);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < s_of.size(); ++i) {
            SampleCols &sc = ds.samples[s_of[i]];
            const uint64_t seq_bytes = 16ull * (blk_at[i + 1] - blk_at[i]) + 32ull;
            sc.d_seq = static_cast<uint8_t *>(colbuf) + col_at[i]; sc.d_qual = sc.d_seq + seq_bytes; sc.d_seq_bytes = seq_bytes;
            sc.d_blk = static_cast<uint32_t *>(blkbuf) + blk_at[i]; sc.n_dev_blk = blk_at[i + 1] - blk_at[i];
            ++T.n_dense_samples;
        }
    }
    return MSNV_OK;
}

int devpack_copy_columns(const SampleCols &sc, uint8_t *dst_seq, uint8_t *dst_qual_bits, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (sc.d_seq_bytes) HIP_TRY(hipMemcpyAsync(dst_seq, sc.d_seq, sc.d_seq_bytes, hipMemcpyDeviceToDevice, st));
    const uint64_t qb = (2 * sc.d_seq_bytes + 7) / 8;
    if (qb) HIP_TRY(hipMemcpyAsync(dst_qual_bits, sc.d_qual, qb, hipMemcpyDeviceToDevice, st));
    return MSNV_OK;
}

// The columns of a dataset whose samples were all packed here (piece layout, not the dense one): a round's buffer already IS the
// dataset's layout for its samples, so one round's buffer is adopted as it stands (no copy at all) and several rounds' are copied
// round by round; a sample whose columns were re-laid behind the pack (deep runs dealt into groups) is copied by itself.
int devpack_place_columns(msnv_dataset &ds, DeviceCols &d, const std::vector<uint64_t> &sbase) {
    hipStream_t st = (hipStream_t)ds.ctx->stream;
    DevPackTables &T = ds.dp;
    const size_t S = ds.samples.size();
    auto in_place = [&](const DevRound &R) {
        for (size_t k = 0; k < R.n_samples; ++k) {
            const SampleCols &sc = ds.samples[R.first_sample + k];
            if (sc.d_seq != R.col_seq + (sbase[R.first_sample + k] - sbase[R.first_sample]) || sc.d_qual != R.col_qual + (sbase[R.first_sample + k] - sbase[R.first_sample]) / 4) return false;
        }
        return sbase[R.first_sample + R.n_samples] - sbase[R.first_sample] == R.seq_total;
    };
    const bool guard = knob::guard_alloc();      // (guarded buffers end at the end of their mapping: no adoption of a buffer that holds two columns)
    if (T.rounds.size() == 1 && T.rounds[0].first_sample == 0 && T.rounds[0].n_samples == S && in_place(T.rounds[0]) && !guard && !knob::no_adopt()) {
        DevRound &R = T.rounds[0];
        d.seq = R.col_seq; d.qual = R.col_qual;
        d.blocks.emplace_back(R.col_buf, R.seq_total + COL_PAD + R.seq_total / 4 + 64);
        d.device_bytes += R.seq_total + COL_PAD + R.seq_total / 4 + 64;
        for (void *&p : T.round_bufs) if (p == R.col_buf) p = nullptr;
        R.col_buf = nullptr;
        T.n_columns_adopted += 1;
        return MSNV_OK;
    }
    if (int rc = dev_alloc((void **)&d.seq, sbase[S] + COL_PAD, &d.device_bytes)) return rc;
    if (int rc = dev_alloc((void **)&d.qual, sbase[S] / 4 + 64, &d.device_bytes)) return rc;
    HIP_TRY(hipMemsetAsync(d.seq + sbase[S], 0xff, COL_PAD, st));
    HIP_TRY(hipMemsetAsync(d.qual + sbase[S] / 4, 0, 64, st));
    for (const DevRound &R : T.rounds) {
        if (!R.n_samples) continue;
        const uint64_t o = sbase[R.first_sample];
        if (in_place(R)) {
            if (R.seq_total) {
                HIP_TRY(hipMemcpyAsync(d.seq + o, R.col_seq, R.seq_total, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(d.qual + o / 4, R.col_qual, R.seq_total / 4, hipMemcpyDeviceToDevice, st));
            }
            continue;
        }
        for (size_t k = 0; k < R.n_samples; ++k) {
            const size_t s = R.first_sample + k;
            const SampleCols &sc = ds.samples[s];
            const uint64_t share = sbase[s + 1] - sbase[s];
            HIP_TRY(hipMemsetAsync(d.seq + sbase[s], 0xff, share, st));
            HIP_TRY(hipMemsetAsync(d.qual + sbase[s] / 4, 0, share / 4, st));
            if (int rc = devpack_copy_columns(sc, d.seq + sbase[s], d.qual + sbase[s] / 4, st)) return rc;
        }
    }
    return MSNV_OK;
}

int devpack_copy_blocks(const SampleCols &sc, uint32_t *dst, void *stream) {
    if (sc.n_dev_blk) HIP_TRY(hipMemcpyAsync(dst, sc.d_blk, sc.n_dev_blk * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MSNV_OK;
}

// devpack_release's share of finalize's state: the events, the wait for kernels that may still read the buffers, the buffers into the batch
void devfin_release(DevPackTables::Fin &f, std::vector<void *> &out) {
    if (f.cov_event) (void)hipEventDestroy((hipEvent_t)f.cov_event);
    if (f.chunk_event) (void)hipEventDestroy((hipEvent_t)f.chunk_event);
    if (f.cov_job || f.cov_tables || !f.keep.empty()) (void)hipDeviceSynchronize();
    for (void *p : {f.cov_job, f.cov_tables, f.cov_tmp, f.tile_base}) if (p) out.push_back(p);
    for (void *p : f.keep) if (p) out.push_back(p);
    f = DevPackTables::Fin{};
}

int devpack_finish(msnv_dataset &ds) {
    if (!ds.dp.ready && ds.dp.round_bufs.empty()) return MSNV_OK;
    if (int rc = devpack_sync_pending(ds)) return rc;
    if (ds.ctx) HIP_TRY(hipStreamSynchronize((hipStream_t)ds.ctx->stream));
    for (SampleCols &sc : ds.samples) { sc.d_seq = nullptr; sc.d_qual = nullptr; }
    devpack_release(ds);
    return MSNV_OK;
}

namespace {
// ------------------------------------------------------------------------------------------ finalize: padding behind the pieces
// The alignment padding behind a piece (up to the next 4 bases) reads as the reference the kernel compares it with, N beyond the tile
// (finalize.cpp: finalize_dataset; msnv_pileup_tiles_narrow32 masks mismatch flags per group of bases, not per base).
__global__ void msnv_fill_padding(const ReadHdr *hdr, const unsigned long long *s_read_base, const unsigned long long *s_seq_base, const uint8_t *s_dev, uint32_t n_samples,
                                  unsigned long long n_pieces, const uint32_t *ref4, uint8_t *seq) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pieces) return;
    uint32_t a = 0, b = n_samples;                       // sample of piece i: last s with s_read_base[s] <= i
    while (b - a > 1) { const uint32_t m = (a + b) / 2; if (s_read_base[m] <= i) a = m; else b = m; }
    if (s_dev && !s_dev[a]) return;                      // (nullptr: every sample was packed on the device)
    const ReadHdr h = hdr[i];
    const uint32_t len = h.cig, stop = (len + 2u * SEQ_ALIGN - 1u) & ~(2u * SEQ_ALIGN - 1u);
    uint8_t *sp = seq + s_seq_base[a] + h.seqoff;
    for (uint32_t j = len; j < stop; ++j) {
        const unsigned long long g = (unsigned long long)h.gpos + j;
        const uint32_t code = (h.gpos % TILE + j < TILE) ? (ref4[g >> 3] >> (4u * (uint32_t)(g & 7u))) & 0xfu : 0xfu;
        const uint32_t sh = (j & 1u) * 4u;
        sp[j >> 1] = (uint8_t)((sp[j >> 1] & ~(0xfu << sh)) | code << sh);
    }
}
}  // namespace

int devpack_fill_padding(DeviceCols &d, const std::vector<uint8_t> &sample_on_device, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!d.n_reads || sample_on_device.empty()) return MSNV_OK;
    bool any = false, all = true;
    for (uint8_t v : sample_on_device) { any |= v != 0; all &= v != 0; }
    if (!any) return MSNV_OK;
    if (all) {
        // nothing to tell the kernel apart by, nothing to free behind it: it runs beside the host's coverage tables (round 5: the wait for it
        // was 0.28 ms of finalize); whoever uses the columns next is on this stream
        hipLaunchKernelGGL(msnv_fill_padding, grid_for(d.n_reads, 256), dim3(256), 0, st, d.hdr, (const unsigned long long *)d.s_read_base, (const unsigned long long *)d.s_seq_base,
                           (const uint8_t *)nullptr, (uint32_t)sample_on_device.size(), (unsigned long long)d.n_reads, d.ref4, d.seq);
        HIP_TRY(hipGetLastError());
        return MSNV_OK;
    }
    DevBuf flags;
    if (int rc = flags.alloc(sample_on_device.size())) return rc;
    HIP_TRY(hipMemcpyAsync(flags.p, sample_on_device.data(), sample_on_device.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(msnv_fill_padding, grid_for(d.n_reads, 256), dim3(256), 0, st, d.hdr, (const unsigned long long *)d.s_read_base, (const unsigned long long *)d.s_seq_base,
                       flags.as<uint8_t>(), (uint32_t)sample_on_device.size(), (unsigned long long)d.n_reads, d.ref4, d.seq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MSNV_OK;
}

// The runtime loads a translation unit's code object when its first kernel is launched (~10 ms): msnv_ctx_create does that here, on the
// thread that brings the context up, instead of inside finalize (devpack.hip: warm_devpack).
__global__ void msnv_warm_devfin() {}
void warm_devfin(void *stream) { hipLaunchKernelGGL(msnv_warm_devfin, dim3(1), dim3(1), 0, (hipStream_t)stream); (void)hipGetLastError(); }

}  // namespace msnv
