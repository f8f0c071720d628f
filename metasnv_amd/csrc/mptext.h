// metasnv_amd/csrc/mptext.h -- `samtools mpileup` TEXT formatted on the device: what mptext.cpp (host side: rounds, tiles, batches, the
// file) and mptext_k.hip (kernels and the HIP calls around them) share.
#pragma once

#include <cstdint>

#include "msnv_internal.h"

namespace msnv {

constexpr int MPT_T = 64;      // positions per tile = lanes of the wavefront that handles one (tile, sample)
constexpr int MPT_B = 64;      // read descriptors a wavefront takes through LDS at a time

// One pushed read (passes the read filters, not depth-capped) of a sample, in file order.  Offsets are relative to the sample's
// record stream; the CIGAR may live in a CG:B,I field behind the qualities (rec_parse), hence its own offset and seq_rel < 0.
struct MptRead { uint64_t cig_off; int32_t pos, end; uint32_t n_cigar; int32_t l_seq, seq_rel; uint32_t flags; };      // flags: mapq | reverse strand << 8
static_assert(sizeof(MptRead) == 32, "descriptors go through LDS as two 16-byte words");
struct MptContig { uint64_t ref_off; int64_t ref_len; uint32_t name_off, name_len; int64_t len; };      // ref_len -1: the contig has no sequence; len: @SQ LN
// positions [t0, t0 + MPT_T) of one contig; lines exist in [vbeg, vend) only (BED).  contig < 0 (MPT_ALL only): an EMPTY tile of contig
// ~contig -- no read list reaches it, every position of [vbeg, vend) is a zero-depth line, and no workgroup walks it (mpt_empty_lines).
struct MptTile { int32_t contig, t0, vbeg, vend; };
struct MptRange { uint32_t lo, hi; };                    // reads of one (tile, sample): from the first with end > t0 to the first with pos >= t0 + MPT_T

// What msnv_mpileup_text_opts asks for, as the kernels' template argument: MPT_ALL -a / -aa (zero-depth lines; which contigs are in play
// is the host's business), MPT_MQ -s (a MAPQ column behind the qualities), MPT_BP -O (a read-offset column behind that).  0: today's text.
enum : uint32_t { MPT_ALL = 1u, MPT_MQ = 2u, MPT_BP = 4u };

// What the kernels of one group of tiles read and write.  The per-cell tables are sample-major: entry s * lines_cap + line.
struct MptJob {
    const uint8_t *const *rec;          // [S] record streams, qualities as the pileup engine sees them
    const MptRead *const *reads;        // [S]
    const MptContig *contigs; const char *ref, *names;
    const MptTile *tiles; const MptRange *ranges;      // [n_tiles], [n_tiles * S]; MPT_ALL: ranges [n_work * S], of the tiles that hold reads
    const uint32_t *work;               // MPT_ALL: [n_work] the tiles of the group that are not empty, ascending (else unused: work item w is tile w)
    uint32_t *cnt, *blen, *rel;         // per cell: kept elements, bases length, offset of the cell behind its line's header
    uint32_t *bplen;                    // MPT_BP: per cell, length of the read-offset column (digits of qpos + 1 and the commas); else NULL
    uint32_t *active, *line_len;        // per line: a pushed read covers the position; bytes of the line (0: no line)
    unsigned long long *line_off;       // [lines + 1] exclusive scan of line_len
    unsigned long long *tile_off;       // [n_tiles + 1] line_off of every tile's first line, the total behind them
    unsigned long long *totals;         // [0] lines, [1] kept elements (cumulative over the call)
    uint32_t *flag;                     // a cell's writer did not end where the next cell starts
    uint32_t S, lines_cap; int32_t min_baseq;
    uint32_t opt;                       // MPT_ALL | MPT_MQ | MPT_BP
};

// mptext_k.hip
// n_work / [work_lo, work_hi): the entries of j.work behind the tiles (MPT_ALL); without it n_work = n_tiles and the two ranges are equal
int  mpt_measure(const MptJob &j, uint32_t n_tiles, uint32_t n_work, void *stream);      // measure, cell offsets, scan: fills everything up to tile_off
int  mpt_write(const MptJob &j, uint32_t tile_lo, uint32_t tile_hi, uint32_t work_lo, uint32_t work_hi, unsigned long long base_off, char *text, void *stream);
int  mpt_pinned_alloc(void **p, uint64_t bytes);
void mpt_pinned_free(void *p);
int  mpt_event_create(void **ev);
void mpt_event_destroy(void *ev);
int  mpt_event_record(void *ev, void *stream);
int  mpt_event_wait(void *ev);                                            // the host waits
int  mpt_stream_wait_event(void *stream, void *ev);
int  mpt_event_ms(void *ev0, void *ev1, double *ms);
int  mpt_copy_to_host_async(void *dst_pinned, const void *src_device, uint64_t bytes, void *stream);

// mptext.cpp
struct MptBed { int32_t n; const int32_t *tid; const int64_t *beg, *end; };
int mptext_records(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params, const MptBed &bed, const uint8_t *const *records,
                   const uint64_t *n_bytes, int32_t n, uint32_t opt, int32_t all_level, char **text, uint64_t *text_bytes, uint64_t stats[8]);
int mptext_files(msnv_ctx *ctx, const char *const *bam_paths, int32_t n_bams, const char *ref_fasta, const char *bed_path, const char *out_path,
                 int32_t host_threads, const msnv_params *params, uint32_t opt, int32_t all_level, uint64_t stats[8]);

}  // namespace msnv
