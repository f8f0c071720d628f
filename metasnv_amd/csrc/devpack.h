// metasnv_amd/csrc/devpack.h -- the per-read stage on the device (devpack.hip): raw BAM alignment records resident in HBM ->
// packed read columns (dataset.h).  What the reference's tools do per read before anything is counted -- samtools' read filters
// (bam_plcmd.c mplp_func [EXT]), its CIGAR walk, the -Q test of every base, qaCompute's read filter and its
// walk over the M blocks (qaCompute.cpp:441-593, the walk :530-552) -- as kernels over a record stream that never visits a host core.
// pack.cpp holds the same stage as host code (MSNV_PACK=host); both produce the same bytes (tests/test_gpu_devpack.py).
#pragma once

#include <cstdint>
#include <vector>

#include "dataset.h"

namespace msnv {

// One round of samples: streams[i] (n_bytes[i] bytes of alignment records, on the host or -- on_device -- in HBM of the dataset's device)
// become ds.samples[first + i].  The headers, intervals and per-sample summaries come back to the host (finalize_dataset builds the tile
// index from them); bases and quality bits stay in HBM.
// in_place_base != NULL (streams on the device, all inside [in_place_base, + in_place_capacity), 16-byte aligned base, 256 readable bytes behind
// the last stream): the records are read where they lie, no copy into a round buffer (qualities may be edited there).
// waits for the round devpack_add_round left running, if any, and takes its last results (dataset.h: DevPackTables::Pending)
int devpack_sync_pending(msnv_dataset &ds);
void devpack_ctx_release(msnv_ctx *ctx);                         // the context's pinned words (msnv_ctx_destroy)
int devpack_add_round(msnv_dataset &ds, size_t first, const uint8_t *const *streams, const uint64_t *n_bytes, int n, bool on_device, const uint8_t *in_place_base = nullptr, uint64_t in_place_capacity = 0);
// A device-packed sample's bases and quality flags as host staging (SampleCols::seq / qual), for the two re-layouts that still run on
// the host (finalize.cpp: relayout_dense, split_deep_runs' relocation).
int devpack_sample_to_host(SampleCols &sc);
int devpack_download_pieces(msnv_dataset &ds);
void devpack_release(msnv_dataset &ds);                       // the pack's tables, round buffers, work buffers; the pinned block back to the context
// msnv_records_deal_device (msnv.h): pack.cpp's records_partition for several streams at once, on the device (devdeal.hip)
int records_deal_device(msnv_ctx *ctx, const uint8_t *const *streams, const uint64_t *n_bytes, int n, bool on_device, const int32_t *owner, int n_contigs, int n_parts,
                        int cov_min_mapq, uint8_t *out, uint64_t capacity, uint64_t gap, uint64_t *part_bytes, msnv_sample_stats *stats, uint64_t *contig_bases);

// pack.cpp: the three sequential edits of the host stage (depth cap, overlapping-mate tweak, snpCall's token limit) for ONE sample whose
// records need them (devpack.hip decides that): per record 1 | pile_ok << 1 | cov_ok << 2 | depth << 16, the stream with the edited
// qualities (empty: nothing was edited), and whether it carries QUAL_CUT marks.
int host_prepass(const msnv_dataset &ds, const uint8_t *rec, uint64_t n_bytes, std::vector<uint32_t> &ovr, std::vector<uint8_t> &patched, bool &cut_marks);

}  // namespace msnv
