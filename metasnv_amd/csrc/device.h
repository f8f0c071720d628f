// metasnv_amd/csrc/device.h -- HBM-resident state of one dataset and the kernel pipeline entry.
#pragma once

#include <cstdint>

#include <string>
#include <unordered_map>
#include <vector>

#include "dataset.h"

namespace msnv {

struct Pair32 { uint32_t x, y; };
// DeviceCols::tile_nslots[] on the device: cells per site row of the tile (<= 16 384 + padding) and, in the top bit, "some sample of the tile
// was split into several pairs": only there can two allele events meet in one cell (finalize.cpp: slots sets it, the scatter half of the tail reads it)
constexpr uint32_t NSLOTS_SPLIT = 1u << 31, NSLOTS_MASK = NSLOTS_SPLIT - 1u;
struct MergedGroupDev { uint64_t hdr_base; uint32_t tile, pair_lo, n_pairs, n_pieces; };   // one merged group of shallow pairs (gather_merged_block): its
                                                                                        // headers in hdr8m, its pairs

// ---- gene / codon annotation tables (ann_tables.cpp builds them, msnv_annotate_sites reads them)
constexpr uint8_t ANN_GENE_MINUS = 1, ANN_GENE_LINEAR = 2;       // strand '-', start < end (call_vC.cpp:609)
struct AnnGene   { int64_t start; int32_t contig; uint32_t flags; };          // start is contig-relative (may be -1)
struct AnnContig { int64_t cg_base, cg_len; uint32_t goff, pad; };            // codon genome: base index, length (-1: absent)
struct AnnHost {
    std::vector<uint32_t> seg_beg, seg_end;     // disjoint, sorted runs of the linear position space
    std::vector<int32_t>  seg_gene;
    std::vector<AnnGene>  genes;
    std::vector<AnnContig> contigs;
    std::vector<uint8_t>  codons;               // 4-bit codes, gene.h numbering A0 T1 C2 G3 N4
};
struct AnnDev {
    uint32_t *seg_beg = nullptr, *seg_end = nullptr; int32_t *seg_gene = nullptr;
    AnnGene *genes = nullptr; AnnContig *contigs = nullptr; uint8_t *codons = nullptr;
    uint32_t n_seg = 0;
    msnv_site_ann *out = nullptr; uint64_t cap_out = 0;
    uint32_t *err = nullptr;                    // [0] first position whose contig has genes but no FASTA record, [1] codon past the end
    bool ready = false;
    std::string key;                            // ann_path + '\n' + fasta_path the tables were built from
    std::vector<std::string> gene_names;
};
int  ann_build(msnv_dataset &ds, const Annotation &an, AnnHost &h);
void ann_gene_names(const Annotation &an, const std::vector<std::string> &contigs, std::vector<std::string> &out);
int  dev_ann_upload(DeviceCols &d, const AnnHost &h);
// Annotates the d.last_sites device site records; err_gpos[k] = UINT32_MAX when error kind k did not occur.
int  dev_annotate(DeviceCols &d, uint32_t n_sites, uint32_t drop_gpos, void *stream, double *ms, uint32_t err_gpos[2]);

// One descriptor per active tile for the gate kernels: everything they look up about their tile in one 64-byte load (finalize.cpp: partial_rows builds them).
// staged: a whole-tile work item leaves the tile's candidates in a record list (then row0 = index of that list); pair_lo / n_plane_pairs:
// the tile's pairs that write allele planes
struct GateTile { uint32_t tile, slot_lo, slot_16, slot_w, slot_hi, vbeg, vend, n_slots; uint64_t row0; uint32_t tot_mode, staged, pair_lo, n_plane_pairs, pad0, pad1; };
static_assert(sizeof(GateTile) == 64, "gate tile descriptor");

// What one pass writes and a pass in flight beside it must not share.  A dataset holds two of these (DeviceCols itself and DeviceCols::alt):
// msnv_pileup_run_many alternates overlapped passes between them.  Allocated, grown and freed as a whole (devmem.hip: passbufs_*), swapped as a whole (kernels.hip: swap_sets).
struct PassBufs {
    uint32_t *tot = nullptr;         // [4][n_tiles*TILE]: mismatching A, C, G, T summed over samples
    uint8_t  *part = nullptr;        // coverage partial row of every work item (tile-major; u16 per position for narrow items, u32 for wide)
    uint8_t  *spill = nullptr;       // [n_pairs][TILE] per-sample coverage, saturating at 255
    uint8_t  *aspill = nullptr;      // [n_pairs][4][TILE] per-sample mismatching A, C, G, T counts (allele planes: noisy reads, finalize.cpp: intermediates); else NULL
    Pair32   *events = nullptr;      // {gpos, sample<<18 | allele<<16 | count}
    Pair32   *overflow = nullptr;    // {gpos, sample<<16 | cov}
    uint32_t *counters = nullptr;    // two blocks of CNT_WORDS ([0] events [1] overflow [2] sites [4] pop lines [5] indiv lines, then the event
                                     // sub-list counters): consecutive passes alternate, the gate kernel of a pass zeroes the other block
    uint32_t  cnt_parity = 0;        // block the NEXT pass uses
    uint32_t *ind4 = nullptr;        // 4 bits per position: some sample holds >= calling_threshold reads of mismatching A / C / G / T
    uint32_t *unc_bits = nullptr;    // 1 bit per position: a sample split into several pairs holds a mismatching allele (follows ind4 in its allocation)
    uint32_t *tile_dirty = nullptr;  // per work item (by the slot of its coverage row), 1 bit per 64 positions of the tile: the item added to the allele totals there
                                     // (set by the pileup kernels, consumed and cleared by the gate)
    uint32_t *unc_sites = nullptr;   // [cap_sites]: sites whose call depends on a split / merged sample's summed counts (msnv_decide_sites)
    unsigned long long *site_row = nullptr;   // per 64 positions: first cell of the first site in them (gate kernel; what an event finds its cell with)
    unsigned long long *site_bits = nullptr;  // 1 bit per position: is a site (written by the gate kernel for every tile)
    uint32_t *site_rank = nullptr;   // per 64 positions: index of their first site (tiles with sites only)
    SiteRec  *sites = nullptr;
    uint32_t *tile_site_base = nullptr, *tile_site_cnt = nullptr;
    unsigned long long *tile_cell_base = nullptr;   // per tile and pass: first cell of its sites' rows (gate kernel)
    uint16_t *ncol = nullptr;        // [4][cap_cells]: mismatching A, C, G, T counts per (site, slot), one column per allele
    uint16_t *cov_col = nullptr;     // [cap_cells]: per-sample coverage.  Structure of arrays: a site's row of cells is contiguous in every column,
                                     // so rows can be zeroed and written 16 bytes at a time; the host zips the five columns into msnv_site_sample records
    uint8_t  *site_flags = nullptr;  // pop_mask | ind_mask << 4
    uint8_t  *site_elig = nullptr;   // alleles still open to the individual rule when the gate kernel has decided what it can (merged gather)
    TileStage *tile_stage = nullptr; // per active tile (index of its GateTile): candidate records of whole-tile work items; behind them, in the same
                                     // allocation, the list of tiles whose candidates did not fit (kernels.hip: stage_ovf_list)
    uint32_t  cap_events = 0, cap_overflow = 0, cap_sites = 0;
    uint64_t  cap_out_sites = 0, cap_cells = 0;
    uint64_t  bytes = 0;             // what the set's buffers hold of DeviceCols::device_bytes
};

struct DeviceCols : PassBufs {
    // ---- inputs (uploaded once by finalize)
    ReadHdr  *hdr = nullptr;         // 16-byte piece headers (wide kernel)
    PieceHdr *hdr8 = nullptr;        // 8-byte tile-local piece headers (narrow32 kernel, MSNV_LAYOUT=pieces; MSNV_HDR4=0 builds)
    uint32_t *hdr4 = nullptr;        // 4-byte chunk-relative piece headers (narrow32 kernel, default; dataset.h: HDR4)
    PieceHdr *hdr8m = nullptr;       // headers of the merged groups of shallow pairs, group by group: pair index in bits 19+, ABSOLUTE seq offset / 8
    uint32_t *tile_pair_merged = nullptr;   // per tile: first merged pair (they sit behind the tile's other pairs)
    uint32_t  n_work_merged = 0;     // work[n_work_narrow .. + n_work_merged) = merged items
    MergedGroupDev *merged_groups = nullptr; uint32_t n_merged_groups = 0;   // every merged group, for the gather
    uint32_t *blk = nullptr;         // dense layout: one descriptor per 32-base block (dense kernel)
    bool      dense = true;
    uint8_t  *seq = nullptr;
    uint8_t  *qual = nullptr;
    uint64_t *s_read_base = nullptr, *s_seq_base = nullptr;   // per sample
    uint32_t *ref4 = nullptr;        // nt16 codes, 8 positions per word, low nibble = lowest position
    uint32_t *ref_lc = nullptr;      // 1 bit per position: FASTA char is a lower-case a/c/g/t
    TilePair *pairs = nullptr;
    uint32_t *tile_pair_start = nullptr;   // n_tiles + 1
    WorkItem *work = nullptr;
    ChunkDesc *chunks = nullptr;
    uint32_t *tile_vbeg = nullptr, *tile_vend = nullptr;   // callable range inside each tile (BED / contig)
    uint32_t  n_tiles = 0, n_pairs = 0, n_work = 0, n_work_narrow = 0, n_samples = 0;   // work[0..n_work_narrow) = narrow items
    uint64_t  n_reads = 0, n_seq_bytes = 0, n_chunks = 0, n_hdr8m = 0, n_blk = 0;
    // ---- intermediates
    uint32_t *active_tiles = nullptr; // tiles that hold work items (gate / gather run over these only)
    uint32_t  n_active_tiles = 0;
    uint64_t *slot_off = nullptr;    // byte offset of every row; n_work + 1
    uint32_t *tile_slot_u16 = nullptr;    // first u16 row of every tile (u8 rows come first)
    uint32_t *tile_slot_wide = nullptr;   // first wide (u32) row of every tile
    uint64_t  part_bytes = 0;
    uint32_t *tile_slot_start = nullptr;   // n_tiles + 1
    bool      allele_planes = false;
    GateTile *gate_tiles = nullptr;  // per active tile
    GateTile *gate_tiles_dense = nullptr, *gate_tiles_staged = nullptr;   // gate_tiles without / only the tiles of whole-tile work items (staged: row0 = index of the record list)
    uint32_t *gather_tiles = nullptr; uint32_t n_gather_tiles = 0;   // active tiles that hold pairs outside merged groups (spill gather)
    uint32_t *tile_stage_idx = nullptr;   // per tile: that index
    uint32_t  max_group_pairs = 0;   // most pairs a merged group holds (<= GMW_PAIRS: the merged gather runs a wavefront per group, kernels.hip)
    uint32_t  n_groups_solo = 0;     // the last n_groups_solo merged groups are whole-tile groups of ONE pair (no gather needed when the pass is fused)
    uint32_t  n_work_fused = 0;      // the last n_work_fused merged work items are whole-tile items
    uint32_t  n_fused_tiles = 0;     // tiles handled by whole-tile work items
    bool      fuse_disabled = false; // the passes of this dataset do not use the record lists (tests, experiments)
    int       qlow_cutoff = 0;       // the -Q cutoff the one-bit quality column was packed with (finalize.cpp: pack_lowq); a pass must ask for the same
    uint32_t  last_ovf_tiles = 0;    // whole-tile work items of the last pass whose candidates did not fit a record list (their tiles took the unfused route)
    bool      wide_tot = false;      // some tile's allele totals need 32 bits per allele (tot_add mode 2): the gate kernel's wide instantiation
    bool      use_dirty = false;     // sparse cohort (few work items per tile): the gate kernel consults tile_dirty before it reads the allele totals
    uint32_t  gather_split = 4;      // workgroups per tile in the spill gather (fewer for sparse cohorts: a pair or two per tile)
    bool      any_split = false;     // some (sample, tile) run was dealt into several pairs: the calling rule then needs the summed per-sample records
    uint32_t *tile_nslots = nullptr; // per tile: samples that have reads in it = cells per site of that tile (kernels.hip: CellMap) | NSLOTS_SPLIT
    uint64_t  last_cells = 0, last_sites = 0;
    // ---- genome coverage (qaCompute path)
    Pair32   *cov_iv = nullptr;          // {gbeg, gend}: +1 at gbeg, -1 at gend (index space of qaCompute.cpp:530-552)
    uint64_t *s_cov_base = nullptr;      // per sample
    TilePair *cov_pairs = nullptr;
    WorkItem *cov_work = nullptr;
    uint32_t *tile_len = nullptr;        // scanned indices of each tile (i < contig length)
    uint32_t *tile_contig_dev = nullptr;
    unsigned long long *cov_acc = nullptr;   // [copy][row][1 + COV_BINS]: covSum, hist[0..] of every (sample, contig) that has intervals (rows: dataset.h); tile t adds to copy t % cov_copies
    uint64_t  n_cov_rows = 0;
    uint32_t  cov_copies = 1;                // (the tiles of a long contig would otherwise queue up on one 64-byte line); summed on the host
    uint32_t  n_cov_pairs = 0, n_cov_work = 0, n_cov_work_wide = 0, n_contigs = 0;   // (the last n_cov_work_wide items hold a pair of > 32 767 intervals)
    uint64_t  n_cov_iv = 0;
    uint64_t  device_bytes = 0;
    uint64_t  algorithmic_bytes = 0;
    // allocations that hold SEVERAL of the tables above (the index arena of finalize, an adopted round buffer of the device pack): pointers
    // into one of them are not freed by themselves (dev_free_all)
    std::vector<std::pair<void *, uint64_t>> blocks;
    AnnDev    ann;
    // second set of per-pass buffers + second stream: msnv_pileup_run_many alternates passes between the two sets so
    // that the small tail kernels of pass i overlap with the pileup kernel of pass i+1 (allocated on first use)
    PassBufs  alt;
    void     *stream2 = nullptr;
    std::vector<void *> event_pool;          // hipEvent_t of msnv_pileup_run_many
    uint32_t *pinned_cnt = nullptr; size_t pinned_cnt_cap = 0;   // pinned host blocks for the per-pass counters
    void     *timing_events[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // hipEvent_t, reused by every pass
};

// host copies of the counters after a run
// The allele-event list is cut into EV_LISTS equal sub-lists, each with its own fill counter on its own 64-byte line
// (work item i appends to sub-list i % EV_LISTS): returning atomics on ONE address serialise device-wide, and reads with
// several per cent of mismatches append often enough for that to dominate the pileup kernel.
constexpr uint32_t EV_LISTS = 32, EV_CNT_STRIDE = 16;
// counters[0..15] (what the host reads back: [0] events [1] overflow [2] sites [4] pop lines [5] indiv lines [6..7] cells), the
// event sub-list counters, then the counters every gate workgroup adds to -- each on a 64-byte line of its own: with a sparse
// cohort 10^5 workgroups add to them, and atomics on one line serialise at the memory side (BASELINE configs[3] shard: the gate
// kernel went from 2.0 to 2.9 ms when two more counters shared the line of the site counter)
constexpr uint32_t CNT_CELLS = 16 + EV_LISTS * EV_CNT_STRIDE;   // 64-bit: cells of the per-sample records
constexpr uint32_t CNT_TALLY = CNT_CELLS + 16;                  // 64-bit: population lines | individual lines << 32 (gate kernel's share)
constexpr uint32_t CNT_UNC = CNT_TALLY + 16;                    // sites left to msnv_decide_sites
constexpr uint32_t CNT_STAGE = CNT_UNC + 8;                   // a whole-tile work item found more than STAGE_CAP candidate positions
constexpr uint32_t CNT_WORDS = CNT_UNC + 16;

struct RunCounts { uint32_t n_events, n_overflow, n_sites, err; uint64_t n_cells; };

// ---- devmem.hip: the current device, the caching allocator, copies, fills and streams
int  dev_set_device(int device);
uint32_t dev_resident_workgroups(uint32_t per_cu);   // compute units of the current device x per_cu (256 CUs when the query fails)
int  dev_alloc(void **p, uint64_t bytes, uint64_t *acct);
void dev_free(void *p);
void dev_free_batch(const std::vector<void *> &ptrs);
int dev_memset_async(void *dst, int v, uint64_t bytes, void *stream);
void dev_cache_trim();                               // cached free blocks back to the runtime (devmem.hip: dev_alloc)
int  dev_upload(void *dst, const void *src, uint64_t bytes);
int  dev_download(void *dst, const void *src, uint64_t bytes);
int  dev_copy_bytes(void *dst_device, const void *src, uint64_t bytes, bool src_on_device, void *stream);      // device <- device or host, on the stream, waited for
int  dev_memset(void *dst, int v, uint64_t bytes);
int  dev_stream_wait(void *stream);
int  dev_stream_create(void **stream);
void dev_stream_destroy(void *stream);

// ---- kernels.hip: one pass of the pipeline (pileup -> gate -> gather -> decide) on `stream`, the coverage pass
constexpr int COV_BINS = 16;            // histogram bins kept on the device (qaCompute -c <= 15)
int  dev_run_coverage(DeviceCols &d, int max_cov, void *stream, msnv_run_stats *stats);
int  dev_coverage_scanned(DeviceCols &d, void *stream, unsigned long long *scanned);      // scanned[n_cov_rows]: positions msnv_coverage_tiles scans per accumulator row
// qaCompute -m / -p / -x from the same index (covext_k.hip).  Rows are the accumulator rows of dataset.h; the host hands over what the kernel
// cannot know (contig lengths, the first tile of every contig, the windows of every row) and takes the medians, window sums and region sums.
constexpr uint32_t CX_BINS = 2048, CX_ROW_WORDS = CX_BINS + 2;      // histogram window of one row + its positions at a negative depth: their number, their sum
struct CovxRegion { uint32_t start, end, max_end, id; };            // per contig sorted by start; max_end: largest end up to here; id: the caller's index
struct CovxJob {
    bool want_median = false; uint32_t window = 0, n_samples = 0;
    std::vector<uint32_t> contig_tile_base;                          // per contig
    std::vector<uint32_t> row_contig;
    std::vector<uint64_t> row_len, row_scanned, row_win_off;          // per row: contig length, positions in tiles with a work item; first window (n_rows + 1)
    std::vector<CovxRegion> regs; std::vector<uint32_t> reg_off;     // regions contig by contig (n_contigs + 1 offsets)
    // results
    std::vector<int32_t> row_median; std::vector<uint64_t> win, reg_sum;      // reg_sum[sample][region id]
    uint32_t n_launches = 0;
};
int  dev_run_coverage_extras(DeviceCols &d, CovxJob &job, void *stream);
int  dev_run_pipeline(DeviceCols &d, const msnv_params &p, void *stream, msnv_run_stats *stats, RunCounts *counts);
int  dev_run_pipeline_many(DeviceCols &d, const msnv_params &p, void *stream, int n, bool overlap, msnv_run_stats *stats, RunCounts *counts);
// ---- devmem.hip again: everything a dataset holds on the device, and its sets of per-pass buffers
void dev_free_all(DeviceCols &d);
// A set of per-pass buffers.  alloc: every buffer of an EMPTY set from the dataset's shape (d's counts; part_bytes, n_active_tiles,
// n_fused_tiles, allele_planes) and the capacities `caps`, the fills queued on `stream`; grow: events, overflow and sites (with unc_sites) to
// what a failed pass asked for; free: everything, and the set's bytes leave d.device_bytes with it.
int  passbufs_alloc(DeviceCols &d, PassBufs &b, const PassBufs &caps, void *stream);
int  passbufs_grow(DeviceCols &d, PassBufs &b, const RunCounts &need);
void passbufs_free(DeviceCols &d, PassBufs &b);
// before a pass: the primary set's output columns hold half as many sites and cells again as the last pass found; before an overlapped
// batch: the second set exists at the first's capacities (its fills queued on `stream` and waited for)
int  ensure_out_for_next_pass(DeviceCols &d);
int  ensure_alt(DeviceCols &d, void *stream);
int  dev_reserve_passes(DeviceCols &d, int n);
// one tiny launch per translation unit with kernels: its code object is loaded when the context is made, not inside the first stage that needs it
void warm_devpack(void *stream), warm_devscan(void *stream), warm_devdeal(void *stream), warm_devfin(void *stream), warm_kernels(void *stream), warm_textcall(void *stream), warm_annotate(void *stream), warm_mptext(void *stream);

// ---- BGZF blocks inflated on the device (inflate_k.hip; bamfeed.cpp drives it)
struct InfBlock { unsigned long long in_off, out_off; uint32_t in_size, out_size; };      // offsets into the batch's compressed / inflated bytes
int  dev_inflate_staging(msnv_ctx *ctx, uint64_t in_bytes, uint64_t out_bytes, uint8_t **in, uint8_t **out);
void dev_inflate_release(msnv_ctx *ctx);
void dev_inflate_release_device(msnv_ctx *ctx);
int  dev_inflate(msnv_ctx *ctx, uint64_t comp_bytes, const std::vector<InfBlock> &blocks, uint64_t out_bytes, std::vector<uint32_t> &status, double *ms_kernel);
int  dev_inflate_device_buffers(msnv_ctx *ctx, uint64_t in_bytes, uint64_t out_bytes);
int  dev_inflate_resident(msnv_ctx *ctx, const uint8_t *host_in, uint64_t comp_bytes, const std::vector<InfBlock> &blocks, const std::vector<uint32_t> &blk_in_file,
                          uint32_t check_every, std::vector<uint32_t> &status, double *ms_kernel);
int  dev_inflate_patch(msnv_ctx *ctx, uint64_t out_off, const uint8_t *data, uint32_t n);

// ---- the stages that work on files (textcall.hip; dist.cpp + dist_k.hip; div.cpp + div_k.hip; subpopr.cpp + subpopr_k.hip; genecorr.cpp + genecorr_k.hip; cluster.cpp + cluster_k.hip; pcoa.cpp + pcoa_k.hip; hclust.cpp + hclust_k.hip; genotype.cpp + genotype_k.hip; profile.cpp + profile_k.hip)
int  text_call(msnv_ctx *ctx, const char *text, uint64_t n_text, const msnv_params &p, const char *ref_fasta, const char *ann_path,
               const char *called_path, const char *indiv_path, uint64_t stats[8]);
int  dist_file(msnv_ctx *ctx, const char *freq_path, const char *mann_path, const char *allele_path, double threshold,
               int32_t *n_samples_out, uint64_t *n_pos_out, double *ms_kernel);
int  div_file(msnv_ctx *ctx, const char *freq_path, int32_t mode, int32_t matched, int64_t genome_length, const double *h, const double *v,
              int32_t n_cov, const int64_t *row_order, uint64_t n_order, const char *out_a, const char *out_b, int32_t *n_samples_out,
              uint64_t *n_rows_out, double *ms_kernel);
int dev_dist(const double *xt_host, int n_samples, long n_pos, double threshold, void *stream, double *mann, double *allele, double *ms_kernel);
// div.cpp + div_k.hip: the rows one position key may hold (m alleles -> k = m(m-1)+1 values per column, k^2 products summed by ONE lane per pair).
// The smaller of (a) what the reference still computes: np.outer allocates 8 k^2 bytes, within 1 GiB up to m = 108 (k = 11 557), MemoryError not far
// beyond; (b) what one lane sums in a second per pair at the measured rate (MEASURED.md "--div / --divNS").  A larger group is refused on the host.
constexpr uint32_t DIV_MAX_ALLELES_REFERENCE = 108, DIV_MAX_ALLELES_DEVICE = 55;
constexpr uint32_t DIV_MAX_ALLELES = DIV_MAX_ALLELES_REFERENCE < DIV_MAX_ALLELES_DEVICE ? DIV_MAX_ALLELES_REFERENCE : DIV_MAX_ALLELES_DEVICE;
int dev_div(const double *xs, const uint64_t *bits, long n_single, long n_words, const double *xg, const long *goff, long n_groups, long n_grouped,
            int n_samples, void *stream, double *out, double *ms_kernel);
int dev_allele_freq(const std::vector<uint32_t> &cov, const std::vector<uint32_t> &cnt, const std::vector<uint32_t> &row_line,
                    uint32_t n_samples, long long min_depth, void *stream, std::vector<double> &freq, double *ms_kernel);
// genecorr.cpp + genecorr_k.hip: subpopr's correlateSubpopProfileWithGeneProfiles.  One workgroup ranks one row of samples in LDS, which bounds the row
constexpr uint32_t GENECORR_MAX_SAMPLES = 8192;
int dev_gene_corr(uint32_t n_clust_rows, uint64_t n_genes, uint32_t n_samples, const double *clust, const double *genes, void *stream, double *rho, double *r,
                  uint8_t *valid, double *pseudocount, double *ms_kernel);
int dev_corr_stats(int method, uint64_t n, const double *est, const int32_t *n_obs, void *stream, double *stat, double *p, double *lo, double *hi, double *q);

// cluster.cpp + cluster_k.hip: subpopr's computeClusters.  The distance matrix of one species, resident on the device for every PAM task run on it
constexpr uint32_t CLUSTER_MAX_SAMPLES = 4096, PAM_MAX_SWAPS = 65536;   // a task that swaps more often than this is refused, not waited for
constexpr uint32_t CLUSTER_BOOT_MAX_K = 32;                             // msnv_cluster_boot: the k x k table of one subset is 4 KB of LDS
struct ClusterDev {
    double *dist = nullptr; uint32_t n = 0;
    ClusterDev() = default;
    ClusterDev(const ClusterDev &) = delete;
    ~ClusterDev();
};
int dev_cluster_upload(ClusterDev &c, const double *dist, uint32_t n, void *stream);
// tasks and splits as include/msnv.h packs them; a split is a list of len global indices whose first floor(len / 2) entries are half 1
int dev_pam_tasks(const ClusterDev &c, uint64_t n_tasks, const uint32_t *m, const uint32_t *k, const int32_t *idx, void *stream, int32_t *med, int32_t *clus,
                  int32_t *swaps, double *ms_kernel);
// task 0 = m[0] members clustered into k, then n_sets subsets (m[1..]; idx as for dev_pam_tasks, pos = each subset entry's position in task 0's list):
// med0[k], clus0[m[0]] and best[n_sets][k][2] = (inter, union) of every original cluster's best match; two launches
int dev_cluster_boot(const ClusterDev &c, uint64_t n_sets, const uint32_t *m, uint32_t k, const int32_t *idx, const int32_t *pos, void *stream, int32_t *med0,
                     int32_t *clus0, int32_t *best, double *ms_kernel);
int dev_pred_strength(const ClusterDev &c, uint64_t n_splits, const uint32_t *len, const uint32_t *k, const int32_t *idx, void *stream, double *prederr, double *ms_kernel);
int dev_freq_bands(const double *rows, uint64_t n_pos, uint32_t n_samples, void *stream, uint64_t *counts, double *ms_kernel);   // counts[sample][4]
// snvfreq.cpp + snvfreq_k.hip: subpopr's snvFreqPlot.  A block of msnv_freq_curves_k is one wavefront of FREQ_CURVE_LANES sample columns over
// FREQ_CURVE_ROWS rows.  counts[sample][102] as msnv_freq_curves lays them out; *outside = 1 when a cell is neither NaN nor within [0, 100]
constexpr uint32_t FREQ_CURVE_LANES = 64, FREQ_CURVE_ROWS = 1024;
int dev_freq_curves(const double *rows, uint64_t n_pos, uint32_t n_samples, double strict_lo, double strict_hi, void *stream, uint64_t *counts, uint32_t *outside,
                    double *ms_kernel);
// snvfreq.cpp, shared with cluster.cpp: the strict band (lo, hi) on the percent scale of subpopr's -x, folded at 0.5
void strict_band(double max_prop_reads_non_homog, double &lo, double &hi);
// cluster.cpp, shared with pcoa.cpp: the checks of a distance matrix (include/msnv.h), the reader of <species>.filtered.mann.dist (r_form: the
// header as write.table prints it), and removeOutliersFromDistMatrixMinDissim(3 sd, at most 5): the samples that stay, in matrix order
int check_matrix(const char *who, int64_t n, const double *d);
int read_dist(const char *path, std::vector<std::string> &names, std::vector<double> &d, bool r_form = false);
std::vector<int32_t> remove_outliers(const std::vector<double> &d, size_t n_all);

// pcoa.cpp + pcoa_k.hip: subpopr's computePCoA, ape::pcoa(correction = "none") by two-sided cyclic Jacobi in round-robin order (include/msnv.h).
// dist: a checked n x n matrix.  Out: eig[n] sorted descending with the cut-off applied, rel_eig[n], axis_pct[n], vectors[n][n_axes] (NaN columns from
// k on), info[8] as msnv_pcoa's.  who names the caller (a species) in the message of a solve that has not settled after PCOA_MAX_SWEEPS sweeps.
constexpr uint32_t PCOA_MAX_SWEEPS = 64;
int dev_pcoa(const char *who, const double *dist, uint32_t n, uint32_t n_axes, void *stream, double *eig, double *rel_eig, double *axis_pct, double *vectors,
             int64_t info[8], double *ms_kernel);
// pcoa.cpp, shared with hclust.cpp: the cell of column `column` per row name, as text, of a table as write.table(sep = '\t', quote = F) prints it
int read_r_column(const std::string &path, const char *column, std::unordered_map<std::string, std::string> &cell);
bool file_exists(const std::string &path);

// hclust.cpp + hclust_k.hip: hclust(method = average | complete | single | mcquitty) of many index lists of one resident matrix, one workgroup of
// HCLUST_THREADS per task (include/msnv.h).  One launch over the tasks given, lists packed as msnv_hclust_tasks packs them; out, per task at
// (the sum of the earlier m) - t: the m - 1 steps (a, b, h) in positions of the list.  The caller cuts a batch by its scratch, 8 * sum(m^2) bytes.
constexpr uint32_t HCLUST_THREADS = 256;
int dev_hclust_batch(const ClusterDev &c, uint64_t n_tasks, const uint32_t *m, const uint32_t *method, const int32_t *idx, void *stream, int32_t *step_a, int32_t *step_b,
                     double *step_h, double *ms_kernel);

// genotype.cpp + genotype_k.hip: subpopr's computeUniquePosPerCluster.  col[] lists the columns in use in cluster order, seg[k] is the first
// entry of cluster k (seg[K] = the list's length).  A row with a mean difference within GENO_GUARD of the threshold is flagged near.
constexpr uint32_t GENO_MAX_CLUSTERS = 32, GENO_MAX_SAMPLES = 65536, GENO_ROWS_PER_BLOCK = 4, GENO_GRID_BLOCKS = 2048;
constexpr uint64_t GENO_SLAB_BYTES = 1ull << 30;
constexpr double GENO_GUARD = 1e-6;
int dev_genotype_rows(const double *rows, uint64_t n_pos, uint32_t n_samples, const uint32_t *col, const uint32_t *seg, uint32_t n_clusters, double threshold,
                      void *stream, uint32_t *select_mask, uint32_t *flip_mask, uint8_t *near_flag, double *ms_kernel);

// profile.cpp + profile_k.hip: subpopr's writeSubpopsForAllSamples.  A workgroup of PROF_WAVES wavefronts owns PROF_COLS adjacent columns; counts[i][s]
// are the called cells, those > 0, >= 5, == 0 and == 100 of column s; *outside: a cell that is neither NaN nor within [0, 100] was seen.
constexpr uint32_t PROF_COLS = 16, PROF_WAVES = 16;
int dev_profile_columns(const double *rows, uint32_t n_rows, uint32_t n_samples, const uint8_t *flip, uint32_t cols_per_pass, void *stream, uint32_t *counts[5],
                        double *mid_lo, double *mid_hi, bool *outside, double *ms_kernel);

}  // namespace msnv
