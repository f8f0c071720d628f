// metasnv_amd/csrc/devfin.h -- finalize's device side (devfin.hip): what finalize.cpp calls for a dataset whose samples were all packed on
// the device (devpack.h).  The per-piece and per-interval loops of finalize_dataset as kernels over the rounds' headers and intervals, which
// never leave HBM; the copies of the rounds' columns into the dataset's; the release of the pack behind finalize's last wait.
// devfin.hip's header has the stages in call order.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "dataset.h"

namespace msnv {

// finalize: copies of the rounds' columns into the dataset's, and the alignment padding behind every piece set to the reference
int devpack_copy_columns(const SampleCols &sc, uint8_t *dst_seq, uint8_t *dst_qual_bits, void *stream);
int devpack_place_columns(msnv_dataset &ds, DeviceCols &d, const std::vector<uint64_t> &sbase);      // fast finalize, piece layout: adopt one round's buffer / copy round by round
int devpack_fill_padding(DeviceCols &d, const std::vector<uint8_t> &sample_on_device, void *stream);
// finalize on the device (all samples device-packed): the per-piece / per-interval loops of finalize_dataset as kernels over the rounds'
// headers and intervals
struct DevMergedSrc { uint32_t pair, in_group; unsigned long long h_base; };   // a pair of a merged group: its index in the group, first slot of its headers in hdr8m
struct DevCovPair { uint32_t tile, sample, lo, hi; };                            // intervals [lo, hi) of `sample` (kept ones, sample-relative) may touch `tile`
int devfin_overhang(msnv_dataset &ds, std::vector<int64_t> &maxend);
// deep (sample, tile) runs (finalize.cpp: split_deep_runs) on the device: exact depth of every run whose bound reaches split_at, runs that are
// really that deep dealt round robin into groups of pieces that each stay below the byte bins' limit; the sample's headers are permuted group
// by group and its columns re-laid in header order.  Updates SampleCols::dev_pairs.  *fallback: a run needs more groups than the kernel holds.
int devfin_deep_runs(msnv_dataset &ds, uint32_t split_at, uint32_t group_depth, bool *fallback);
// finalize.cpp: relayout_dense for device-packed samples: every sample's columns as dense block streams, its descriptors (d_blk) and run_* tables
int devfin_dense(msnv_dataset &ds);
int devpack_copy_blocks(const SampleCols &sc, uint32_t *dst, void *stream);
int devfin_headers(msnv_dataset &ds, DeviceCols &d, const std::vector<uint64_t> &rbase);
// the narrow pairs' chunks (d.chunks, d.hdr4) cut without a wait: item_first[wi] = index of narrow work item wi's first pair in the list (n_work_narrow + 1 entries); the chunks
// go behind the `base` chunks the host wrote, `cap` of them at most; devfin_chunks_result (behind a wait for the stream) says how many there were
int devfin_chunks_launch(msnv_dataset &ds, DeviceCols &d, const std::vector<uint32_t> &narrow_pairs, const std::vector<uint32_t> &item_first, uint32_t base, uint64_t cap);
int devfin_chunks_result(msnv_dataset &ds, uint64_t *n_chunks, bool *overflow);
int devfin_work_first(msnv_dataset &ds, DeviceCols &d, uint32_t n_items, uint64_t n_room);         // WorkItem::first of the narrow and merged items, from d.chunks (n_room descriptors)
int devfin_merged_headers(msnv_dataset &ds, DeviceCols &d, const std::vector<DevMergedSrc> &list);
int devfin_coverage_launch(msnv_dataset &ds, DeviceCols &d);   // needs ds.tile_base / n_tiles; the kernels only (their results: devfin_coverage)
int devfin_coverage(msnv_dataset &ds, DeviceCols &d, std::vector<uint64_t> &cvbase, std::vector<DevCovPair> &cp);
// waits for the copies, releases the round buffers and the tables (no sample can be added after finalize)
int devpack_finish(msnv_dataset &ds);
// devpack_release's share of finalize's state (DevPackTables::Fin): destroys its events, waits for the device when kernels that read its
// buffers may still be queued, appends the buffers to the batch devpack_release frees.  Leaves `f` as a fresh dataset has it.
void devfin_release(DevPackTables::Fin &f, std::vector<void *> &out);

// The second half of the dataset's pinned block while finalize runs: the small results its kernels leave for the host, as 32-bit words.
// Region after region, none sized by anything but S (the samples): ONE pin_ensure(ds, FinWords::bytes(S)) at finalize's
// first use covers every later one, so the block is never grown -- swapped -- while copies into it are queued.
struct FinWords {
    uint32_t *w = nullptr; size_t S = 0;
    static constexpr size_t n_kept(size_t S) { return S + 3; }
    static constexpr size_t kept_at(size_t) { return 0; }                                      // n_kept words
    static constexpr size_t chunks_at(size_t S) { return kept_at(S) + n_kept(S); }             // 2
    static constexpr size_t tables_at(size_t S) { return chunks_at(S) + 2; }                   // 4
    static constexpr size_t row_start_at(size_t S) { return tables_at(S) + 4; }                // S + 1
    static constexpr size_t words(size_t S) { return row_start_at(S) + S + 1; }
    static constexpr uint64_t bytes(size_t S) { return (uint64_t)words(S) * 4; }
    // the coverage index launched ahead: kept intervals before every sample [0 .. S], kept in all [S + 1], (sample, tile) runs [S + 2]
    uint32_t *kept() const { return w + kept_at(S); }
    uint32_t &n_runs() const { return w[kept_at(S) + S + 2]; }
    // the chunk cut: [0] narrow chunks in all, [1] more than there was room for
    uint32_t *chunks() const { return w + chunks_at(S); }
    // the coverage pair tables: [0] pairs [1] accumulator rows [2] work items [3] some pair is wide
    uint32_t *tables() const { return w + tables_at(S); }
    uint32_t *row_start() const { return w + row_start_at(S); }                                // S + 1 words: first row of every sample, the rows in all
};
// (no two regions overlap, whatever S: every region starts where the one before it ends, and is at least as long as what is kept there)
constexpr bool fin_words_disjoint(size_t S) {
    return FinWords::chunks_at(S) >= FinWords::kept_at(S) + FinWords::n_kept(S) && FinWords::tables_at(S) >= FinWords::chunks_at(S) + 2 &&
           FinWords::row_start_at(S) >= FinWords::tables_at(S) + 4 && FinWords::words(S) >= FinWords::row_start_at(S) + S + 1;
}
constexpr bool fin_words_disjoint_upto(size_t n) { for (size_t S = 0; S <= n; ++S) if (!fin_words_disjoint(S)) return false; return true; }
static_assert(fin_words_disjoint_upto(64) && fin_words_disjoint(16383) && fin_words_disjoint(16384), "FinWords: regions overlap");

}  // namespace msnv
