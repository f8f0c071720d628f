// metasnv_amd/csrc/knobs.h -- every MSNV_* environment knob of libmsnv.so, declared once: name, kind, default and clamp, WHEN it is
// read, and what for.  The only file of csrc/ that calls getenv (tools/ excepted); tests/test_knobs.py holds it to that, to one string
// literal per name, and to the table of KERNELS.md "Environment knobs".  The Python side's names live in metasnv_amd/knobs.py.
//
// When a knob is read:
//   once       function-local static in the accessor: the first call of the process decides.  A test sets it for a child process.
//   per call   not cached: every call of the accessor reads the environment ("per dataset", "per pass", "per round" say which call of
//              the library that is).  A test may set it inside a live process.
// What counts as "on" is what each site always took and differs by knob: a first character ('1', '0' or the first letter of a word:
// MSNV_PACK=host and MSNV_PACK=h are the same), mere presence (then =0 switches it ON too; the comment says "present"), or an integer
// with atoi / atoll semantics (an empty string or junk is 0, then the clamp applies).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace msnv {
namespace knob {

// ---------------------------------------------------------------------------------- the three ways a value is taken
inline char first(const char *name) { const char *e = getenv(name); return e ? e[0] : '\0'; }      // '\0': unset or empty
inline bool present(const char *name) { return getenv(name) != nullptr; }
inline bool int_of(const char *name, int *v) { const char *e = getenv(name); if (e) *v = atoi(e); return e != nullptr; }            // false (and *v as it was): unset
inline bool i64_of(const char *name, long long *v) { const char *e = getenv(name); if (e) *v = atoll(e); return e != nullptr; }
inline int       int_or(const char *name, int dflt) { int_of(name, &dflt); return dflt; }
inline long long i64_or(const char *name, long long dflt) { i64_of(name, &dflt); return dflt; }

// ---------------------------------------------------------------------------------- host IO and inflate (hostio.cpp, crc32.cpp, bamfeed.cpp, inflate_k.hip)
// MSNV_INFLATE_CHECK=n: block i of a file is checked against the CRC-32 of its BGZF trailer when i % n == 0 (default 1: every block, as
// htslib does; 0 or negative: none -- benchmarks).  ONE reading for the host decoder and the device inflate.  Per call (tests/test_crc32.py,
// test_hostio.py, test_gpu_inflate*.py switch it).
inline uint32_t inflate_check_every() { const int v = int_or("MSNV_INFLATE_CHECK", 1); return (uint32_t)(v < 0 ? 0 : v); }
// MSNV_INFLATE=device|host|zlib has TWO readings.  (1) Where a call's BGZF blocks are inflated: 'd' the device whatever the size, any other
// value ('h') the host, '\0' unset = bamfeed.cpp estimates.  Per call (tests/test_gpu_inflate.py and bench.py switch device / host in process).
constexpr const char *INFLATE = "MSNV_INFLATE";
inline char inflate_where() { const char *e = getenv(INFLATE); return !e ? '\0' : e[0] == 'd' ? 'd' : 'h'; }
// (2) 'z': the host decoder hands every block to zlib (A/B of the two decoders).  Once: asked per BGZF block by many threads; set for a
// child only (tests/test_inflate.py).
inline bool inflate_zlib() { static const bool on = first(INFLATE) == 'z'; return on; }
// MSNV_INFLATE_BATCH_MB: compressed megabytes per batch of the device inflate (default 1024, 2048 for the resident form; at least 1).
// Per call (tests/test_gpu_inflate.py).  metasnv_amd/knobs.py: inflate_batch_mb restates the 1024.
inline uint64_t inflate_batch_bytes(bool resident = false) { return (uint64_t)std::max<long long>(1, i64_or("MSNV_INFLATE_BATCH_MB", resident ? 2048 : 1024)) << 20; }
// MSNV_TEST_NO_STAGING=1: the device inflate's pinned staging is refused, the host takes the batch.  Per call (tests/test_gpu_inflate.py).
inline bool test_no_staging() { return first("MSNV_TEST_NO_STAGING") == '1'; }
// MSNV_TEST_RESIDENT_FAIL (present): the resident inflate is refused, the staged form takes over.  Per call (tests/test_gpu_inflate.py).
inline bool test_resident_fail() { return present("MSNV_TEST_RESIDENT_FAIL"); }
// MSNV_CRC=table: the CRC-32 by table lookups although the CPU has carry-less multiply.  Once, when the library is loaded (tests/test_crc32.py: a child).
inline bool crc_table() { static const bool on = first("MSNV_CRC") == 't'; return on; }
// MSNV_HUGE (1): 0 = small pages for the large host buffers, 2 = huge pages populated at once.  Once.  Profiling only (profiles/stage_threads.py).
inline int huge_pages() { static const int mode = int_or("MSNV_HUGE", 1); return mode; }
// MSNV_FINALIZE_TRACE=1, MSNV_FEED_TRACE=1: wall seconds of finalize's / the BAM feed's stages to stderr.  Once
// (tests/test_gpu_finalize_routes.py reads the trace of a child: tests/_route_worker.py; the feed trace is profiling only).
inline bool finalize_trace() { static const bool on = first("MSNV_FINALIZE_TRACE") == '1'; return on; }
inline bool feed_trace() { static const bool on = first("MSNV_FEED_TRACE") == '1'; return on; }
// MSNV_STAGE_FREE=s|n: the staged streams' buffers are freed on the caller's thread ('s') or never ('n'); '\0' = by helper threads.
// Per call.  Profiling only.
inline char stage_free() { const char c = first("MSNV_STAGE_FREE"); return c == 's' || c == 'n' ? c : '\0'; }

// ---------------------------------------------------------------------------------- the per-read stage (api.cpp, bamfeed.cpp, devscan.hip, devpack.hip)
// MSNV_PACK=host: BAM records are packed by the host stage (pack.cpp) although the dataset has a context.  Per call (tests/test_gpu_devpack.py, bench.py).
inline bool pack_on_host() { return first("MSNV_PACK") == 'h'; }
// MSNV_PACK_ROUND_MB (6144, at least 1): record megabytes per round of the device pack.  Per call (tests/test_gpu_devpack.py).
inline uint64_t pack_round_bytes() { return (uint64_t)std::max<long long>(1, i64_or("MSNV_PACK_ROUND_MB", 6144)) << 20; }
// MSNV_PACK_COPY (present): record streams that are already in HBM are copied into the round's buffer, not packed in place.  Per call.  Profiling only.
inline bool pack_copy() { return present("MSNV_PACK_COPY"); }
// MSNV_SCAN=segments: record boundaries by the careful kernel only, no sub-segment walk.  Per call (tests/test_gpu_devpack.py, test_gpu_record_walk.py, fuzz_parity.py).
inline bool scan_segments() { return first("MSNV_SCAN") == 's'; }
// MSNV_FRONT=careful: a round takes the stage-by-stage route, not the one-walk route.  Per call (tests/test_gpu_devpack.py, test_gpu_record_walk.py).
inline bool front_careful() { return first("MSNV_FRONT") == 'c'; }
// MSNV_SCAN_SUB (64 .. 32768): bytes of a sub-segment of the boundary walk.  Its default belongs to the route that asks: 4096 in
// scan_sub_walk (the deal, the careful route), 6144 in a round's one-walk route (2.36 -> 2.04 ms of scan + measure on the benchmark shape
// against 4 KB, 8 KB the same).  Per call (tests/test_gpu_devpack.py and test_gpu_record_walk.py set it).
constexpr long long SCAN_SUB_STREAMS = 4096, SCAN_SUB_ROUND = 6144;
inline uint32_t scan_sub_bytes(long long route_default) { return (uint32_t)std::min<long long>(32768, std::max<long long>(64, i64_or("MSNV_SCAN_SUB", route_default))); }
// MSNV_SCAN_SEG_KB (256, at least 1): kilobytes of a segment of the careful boundary scan.  Per call (tests/test_gpu_devpack.py shrinks it).
inline uint64_t scan_seg_bytes() { return (uint64_t)std::max<long long>(1, i64_or("MSNV_SCAN_SEG_KB", 256)) << 10; }
// MSNV_TILE_ORDER=sort: every round through the rocPRIM sort of the tile order.  Per round (tests/test_gpu_finalize_routes.py::test_per_read_stage_knob).
inline bool tile_order_sort() { return first("MSNV_TILE_ORDER") == 's'; }
// MSNV_DEPTH_STREAM=main: the depth stage in front of the emit kernels, on their stream (A/B).  Once
// (tests/test_gpu_finalize_routes.py::test_knobs_read_once_per_process: a child).
inline bool depth_on_main() { static const bool on = first("MSNV_DEPTH_STREAM") == 'm'; return on; }
// MSNV_OVERLAP=host: the overlaps of a round's pieces by the host.  Per round (tests/test_gpu_devpack.py).
inline bool overlap_on_host() { return first("MSNV_OVERLAP") == 'h'; }
// MSNV_PREPASS=host: the depth cap and snpCall's token limit by pack.cpp's host pre-pass, not msnv_cap_reads / msnv_token_cut.
// Per round (tests/test_gpu_devpack.py, test_gpu_parity.py).
inline bool prepass_on_host() { return first("MSNV_PREPASS") == 'h'; }
// MSNV_EMIT=slow: every block through msnv_emit_block_slow.  Per round (tests/test_gpu_devpack.py).
inline bool emit_slow() { return first("MSNV_EMIT") == 's'; }
// MSNV_DEBUG_SYNC (present): a wait behind every kernel of the emit stage (finds the kernel behind a memory fault).  Once.
// Debugging only (no test sets it).
inline bool debug_sync() { static const bool on = present("MSNV_DEBUG_SYNC"); return on; }
// MSNV_NO_ADOPT (present): a single round's columns are copied, not adopted.  Per dataset (tests/test_gpu_finalize_routes.py::test_per_read_stage_knob).
inline bool no_adopt() { return present("MSNV_NO_ADOPT"); }

// ---------------------------------------------------------------------------------- finalize: layout and deep runs (finalize.cpp)
// MSNV_LAYOUT=pieces|dense: 'p' / 'd' force the per-piece / the dense block layout; '\0' = by the mean piece length.  Per dataset
// (tests/test_gpu_devpack.py, test_gpu_finalize_routes.py).
inline char layout() { const char c = first("MSNV_LAYOUT"); return c == 'p' || c == 'd' ? c : '\0'; }
// MSNV_DEEP=wide: deep (sample, tile) runs stay whole for msnv_pileup_tiles_wide.  Per dataset (tests/test_gpu_parity.py).
inline bool deep_wide() { return first("MSNV_DEEP") == 'w'; }
// MSNV_SPLIT_AT (192; 32 .. max_depth = NARROW_MAX_DEPTH), MSNV_GROUP_DEPTH (128; 16 .. 250): depth from which a run is dealt into groups,
// and the depth a group may reach.  Per dataset, like MSNV_DEEP (tests/test_gpu_devpack.py sets both in process).
inline uint32_t split_at(int max_depth) { return (uint32_t)std::min(max_depth, std::max(32, int_or("MSNV_SPLIT_AT", 192))); }
inline uint32_t group_depth() { return (uint32_t)std::min(250, std::max(16, int_or("MSNV_GROUP_DEPTH", 128))); }
// MSNV_DEEP_RELOCATE=0: the bases / qualities of a sample dealt into groups stay in read order (host loops of finalize; A/B).
// Per dataset (tests/test_gpu_finalize_routes.py::test_per_read_stage_knob).
inline bool deep_relocate_off() { return first("MSNV_DEEP_RELOCATE") == '0'; }
// MSNV_FINALIZE=host, MSNV_DENSE_RELAYOUT=host: the tile index of a device-packed dataset / the dense re-layout of short reads by the
// host loops of finalize.  Per dataset (tests/test_gpu_devpack.py; tests/test_gpu_finalize_routes.py::test_per_read_stage_knob).
inline bool finalize_on_host() { return first("MSNV_FINALIZE") == 'h'; }
inline bool dense_relayout_on_host() { return first("MSNV_DENSE_RELAYOUT") == 'h'; }
// MSNV_FILL_PADDING (present): the padding nibbles by finalize's kernel although the emit kernels left them.  Per dataset (tests/test_gpu_devpack.py).
inline bool fill_padding() { return present("MSNV_FILL_PADDING"); }

// ---------------------------------------------------------------------------------- finalize: work items (finalize.cpp)
// MSNV_SHALLOW_PIECES (48, at least 0): pieces up to which a pair is merged into a group, 0 = never.  Per dataset (tests/test_gpu_parity.py).
inline uint32_t shallow_pieces() { return (uint32_t)std::max(0, int_or("MSNV_SHALLOW_PIECES", 48)); }
// MSNV_MERGE_ALWAYS=1: merge even when the shallow pairs hold < 3 % of the pieces.  Per dataset (tests/test_gpu_devpack.py, test_gpu_parity.py).
inline bool merge_always() { return first("MSNV_MERGE_ALWAYS") == '1'; }
// MSNV_FUSE=0|1: whole-tile work items off / on whatever the cohort looks like; '\0' = sparse cohorts only.  MSNV_FUSE_PIECES (256, at
// least 1): pieces a pair may hold to take part.  Per dataset (tests/test_gpu_devpack.py; tests/test_gpu_finalize_routes.py::test_per_read_stage_knob).
inline char fuse() { const char c = first("MSNV_FUSE"); return c == '0' || c == '1' ? c : '\0'; }
inline uint32_t fuse_pieces() { return (uint32_t)std::max(1, int_or("MSNV_FUSE_PIECES", 256)); }
// MSNV_ITEM_PIECES (2000; at least 64, a negative value is a huge one): pieces per pileup work item.  Per dataset (tests/test_gpu_parity.py).
inline uint64_t item_pieces() { return std::max<uint64_t>(64, (uint64_t)i64_or("MSNV_ITEM_PIECES", 2000)); }
// MSNV_ITEM_TAPER=0: no taper of the last tiles' work items.  MSNV_TAPER_AT=u1,u2,u3 (1.8,0.73,0.27): the taper's thresholds in full
// waves of workgroups; fields that do not parse keep their defaults.  Per dataset (tests/test_gpu_parity.py).
inline bool item_taper() { return first("MSNV_ITEM_TAPER") != '0'; }
struct TaperAt { double u1 = 1.8, u2 = 0.73, u3 = 0.27; };
inline TaperAt taper_at() { TaperAt t; if (const char *e = getenv("MSNV_TAPER_AT")) sscanf(e, "%lf,%lf,%lf", &t.u1, &t.u2, &t.u3); return t; }
// MSNV_TOT_MODE (0; 0 .. 2): narrowest allele-total layout allowed.  Per dataset (tests/test_gpu_parity.py runs every width on every tile).
inline uint32_t tot_mode_min() { return (uint32_t)std::min(2, std::max(0, int_or("MSNV_TOT_MODE", 0))); }
// MSNV_GATHER_SPLIT (at least 1; default: by the dataset's pairs per tile): parts a tile's gather is split into.  Per dataset (tests/test_gpu_parity.py).
inline uint32_t gather_split(uint32_t by_dataset) { int v = 0; return int_of("MSNV_GATHER_SPLIT", &v) ? (uint32_t)std::max(1, v) : by_dataset; }
// MSNV_CHUNK_CAP (at least 0; default: the bound of the dataset's pairs): slots of the device-cut chunk table; too few force the second
// cut with the exact count.  Per dataset (tests/test_gpu_finalize_routes.py::test_chunk_table_overflow_*).
inline uint64_t chunk_cap(uint64_t bound) { long long v = 0; return i64_of("MSNV_CHUNK_CAP", &v) ? (uint64_t)std::max<long long>(0, v) : bound; }
// MSNV_ALLELES=planes|events: 'p' allele planes, any other value ('e') events, '\0' unset = by the sampled mismatch rate.
// Per dataset (tests/test_gpu_parity.py, test_gpu_stress.py).
inline char alleles() { const char *e = getenv("MSNV_ALLELES"); return !e ? '\0' : e[0] == 'p' ? 'p' : 'e'; }
// MSNV_CAP_EVENTS (at least min_events = EV_LISTS; default: by the dataset's sampled mismatches): first capacity of the allele-event
// list.  Per dataset (tests/test_gpu_parity.py forces the grow-and-rerun path).
inline uint32_t cap_events(uint32_t by_dataset, long long min_events) { long long v = 0; return i64_of("MSNV_CAP_EVENTS", &v) ? (uint32_t)std::max(min_events, v) : by_dataset; }

// ---------------------------------------------------------------------------------- finalize: the coverage index (finalize.cpp, devfin.hip)
// MSNV_COV_INDEX=sort|dense: 'd' the dense table / 's' the sort form whatever the dataset's size; '\0' = by size.  Per dataset
// (tests/test_gpu_finalize_routes.py::test_coverage_index_route).
inline char cov_index() { const char c = first("MSNV_COV_INDEX"); return c == 'd' || c == 's' ? c : '\0'; }
// MSNV_COV_LATE (present): the dense table inside devfin_coverage, waiting, not launched ahead.  MSNV_COV_TABLES=host: pair tables, rows and
// work items by finalize.cpp's host loops (coverage_tables).  MSNV_COV_THREAD (present): the host's tables on a helper thread (measured slower).  Per dataset
// (tests/test_gpu_finalize_routes.py::test_coverage_index_route).
inline bool cov_late() { return present("MSNV_COV_LATE"); }
inline bool cov_tables_on_host() { return first("MSNV_COV_TABLES") == 'h'; }
inline bool cov_thread() { return present("MSNV_COV_THREAD"); }
// MSNV_COV_ITEM (16384; 0 or negative = the default; at most 2^31 - 1): intervals at which a coverage work item is cut before it holds
// COV_ITEM_PAIRS pairs.  MSNV_COV_NARROW_MAX (32767; 1 .. 32767): intervals of a pair above which its item runs in
// msnv_coverage_tiles<true>.  ONE reading each for the host's and the device's tables, which must come out byte-identical.
// Per dataset (tests/test_gpu_parity.py; tests/test_gpu_finalize_routes.py sets 1 to run everything through the wide variant).
inline uint32_t cov_item_intervals() { const long long v = i64_or("MSNV_COV_ITEM", 16384); return (uint32_t)std::min<long long>(v > 0 ? v : 16384, 0x7fffffffll); }
inline uint32_t cov_narrow_max() { return (uint32_t)std::min<long long>(32767, std::max<long long>(1, i64_or("MSNV_COV_NARROW_MAX", 32767))); }

// ---------------------------------------------------------------------------------- the pass (kernels.hip) and the allocator (devmem.hip)
// MSNV_MERGED_GATHER=block|wave: 1 a workgroup / 2 a wavefront per merged group; 0 = by the dataset's groups.  Per pass (tests/fuzz_parity.py).
inline int merged_gather() { const char c = first("MSNV_MERGED_GATHER"); return c == 'b' ? 1 : c == 'w' ? 2 : 0; }
// MSNV_LEAN=0: whole-tile work items through the ordinary body of msnv_pileup_tiles_narrow32.  Per pass (tests/test_gpu_parity.py::test_whole_tile_work_items).
inline bool lean_off() { return first("MSNV_LEAN") == '0'; }
// MSNV_GATE_TILES (1 .. max_tiles = GATE_MAX_TILES; default: by the number of active tiles): tiles per workgroup of msnv_gate_sites.
// Per pass (tests/test_gpu_parity.py).
inline uint32_t gate_tiles(uint32_t by_tiles, int max_tiles) { int v = 0; return int_of("MSNV_GATE_TILES", &v) ? (uint32_t)std::min(max_tiles, std::max(1, v)) : by_tiles; }
// MSNV_TAIL_SKIP (0): bit mask of tail kernels a pass leaves out (timing by omission; the results are wrong).  Once.  Profiling only.
inline uint32_t tail_skip() { static const uint32_t v = (uint32_t)int_or("MSNV_TAIL_SKIP", 0); return v; }
// MSNV_SCATTER_BLOCKS (default_blocks = SCATTER_BLOCKS_PER_LIST; at least 1): workgroups per event list of the gather / scatter launch.
// Once (tests/test_gpu_finalize_routes.py::test_knobs_read_once_per_process at 1 and 64: a child each).
inline uint32_t scatter_blocks(uint32_t default_blocks) { static const uint32_t v = [&] { int x = 0; return int_of("MSNV_SCATTER_BLOCKS", &x) ? (uint32_t)std::max(1, x) : default_blocks; }(); return v; }
// MSNV_PHASE_TIMES=1: HIP events between the tail kernels (~6 us each).  Once.  Profiling only (profiles/phase_times.py).
inline bool phase_times() { static const bool on = first("MSNV_PHASE_TIMES") == '1'; return on; }
// MSNV_GUARD_ALLOC=1: every device buffer ends at the end of its own mapping with unmapped addresses behind it, so that an access past
// its end faults.  Once (tests/test_gpu_guard.py sets it for a child).
inline bool guard_alloc() { static const bool on = first("MSNV_GUARD_ALLOC") == '1'; return on; }
// MSNV_GUARD_FILL=n: fresh guarded mappings are filled with byte n (false: unset, no fill).  MSNV_GUARD_LOG (present): one line per
// guarded allocation to stderr.  Per allocation (tests/test_gpu_guard.py sets the fill for a child; the log is debugging only).
inline bool guard_fill(int *byte) { return int_of("MSNV_GUARD_FILL", byte); }
inline bool guard_log() { return present("MSNV_GUARD_LOG"); }
// MSNV_DEV_CACHE_MB (at least 0; -1 unset = a sixteenth of the device's memory, at most 16 GB): megabytes of freed device blocks the
// caching allocator keeps; 0 = no cache.  Once.  Profiling only.
inline long long dev_cache_mb() { static const long long mb = [] { long long v = 0; return i64_of("MSNV_DEV_CACHE_MB", &v) ? std::max<long long>(0, v) : -1ll; }(); return mb; }

// ---------------------------------------------------------------------------------- the mpileup-text kernel (textcall.hip)
// MSNV_TEXT_CHUNK (default_bytes; at least 1, a negative value is a huge one): bytes of mpileup text per launch.  Per call
// (tests/test_gpu_mpileup_text*.py use a few hundred).
inline uint64_t text_chunk_bytes(uint64_t default_bytes) { long long v = 0; return i64_of("MSNV_TEXT_CHUNK", &v) ? std::max<uint64_t>(1, (uint64_t)v) : default_bytes; }
// MSNV_TEXT_REPEAT (1, at least 1): n - 1 untimed launches before the timed one.  Per call.  Profiling only (profiles/text_bench.py).
inline int text_repeat() { return std::max(1, int_or("MSNV_TEXT_REPEAT", 1)); }

// ---------------------------------------------------------------------------------- the mpileup-text writer (mptext.cpp)
// MSNV_MPTEXT_BATCH (64 MB; at least 1): bytes of text per batch that leaves the device (whole tiles; a tile that is longer is a batch
// of its own).  Per call (tests/test_gpu_mpileup_write.py sets a few bytes and a few kilobytes).
inline uint64_t mptext_batch_bytes() { return (uint64_t)std::max<long long>(1, i64_or("MSNV_MPTEXT_BATCH", 64ll << 20)); }
// MSNV_MPTEXT_ROUND (64, at least 1): samples per round -- pre-pass on the host threads, one upload.  Per call (tests/test_gpu_mpileup_write.py).
inline int mptext_round_samples() { return std::max(1, int_or("MSNV_MPTEXT_ROUND", 64)); }

// ---------------------------------------------------------------------------------- the file stages' row slabs (stagedev.h)
// MSNV_STAGE_SLAB_ROWS=n (0: no cap; a negative value is 0): a row slab of dev_genotype_rows, dev_freq_bands, dev_freq_curves and dev_gene_corr
// holds at most n rows, so that a table of a few rows walks several slabs.  Per call (tests/test_gpu_stage_slabs.py, tests/test_gpu_snvfreq.py).
inline uint64_t stage_slab_rows() { return (uint64_t)std::max<long long>(0, i64_or("MSNV_STAGE_SLAB_ROWS", 0)); }

// ---------------------------------------------------------------------------------- the hclust batches (hclust.cpp)
// MSNV_HCLUST_SCRATCH_KB (1048576 = 1 GiB; at least 1): kilobytes of gathered sub-matrices, 8 m^2 bytes per task, that one launch of
// msnv_hclust_tasks_k may hold; a task that is larger is a launch of its own.  Per call (tests/test_gpu_hclust.py sets 1 to cut a batch).
inline uint64_t hclust_scratch_bytes() { return (uint64_t)std::max<long long>(1, i64_or("MSNV_HCLUST_SCRATCH_KB", 1ll << 20)) << 10; }

}  // namespace knob
}  // namespace msnv
