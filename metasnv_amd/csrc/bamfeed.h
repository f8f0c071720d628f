// metasnv_amd/csrc/bamfeed.h -- the host side of the BAM feed (bamfeed.cpp): files read, BGZF blocks indexed, inflated on the device
// (inflate_k.hip) or by the host decoder, checked, handed to a consumer batch by batch; and the pool of host threads api.cpp shares with it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "device.h"

namespace msnv {

// `threads` host threads (at most one per `grain` indices) take `grain` indices of [lo, hi) at a time and call body(i) for each.  A body that
// returns a code (its message in msnv_last_error()) or throws (MSNV_ENOMEM "<name_of(i)>: <what>") ends the job: no new index is taken, and
// the call fails with the code AND the message of the LOWEST failing index.  timer: a HostTimer every worker runs under (thread-seconds).
int for_each_index(size_t lo, size_t hi, int threads, size_t grain, const std::function<int(size_t)> &body,
                   const std::function<std::string(size_t)> &name_of, int timer = -1);
// threads of a call: the caller's wish or the machine's, at most one per item
int pool_threads(int host_threads, int n);

bool file_size(const char *path, uint64_t *n);      // false: the file cannot be opened or sized (the callers word that, or skip the file)

// metaSNV assumes every BAM shares the header of the first (metaSNV.py:82-83)
int check_header(const msnv_dataset &ds, const BamHeader &h, const char *path);

// n streams appended as n samples through the device pack (devpack.hip), in rounds of at most MSNV_PACK_ROUND_MB of record bytes; and what a
// call does that appends its samples in SEVERAL such calls when a later one fails (the samples of the earlier ones go too, the dataset is poisoned)
int add_streams_device(msnv_dataset *ds, const uint8_t *const *records, const uint64_t *n_bytes, int n, bool streams_on_device,
                       const uint8_t *in_place_base = nullptr, uint64_t in_place_capacity = 0);
int fail_multi_add(msnv_dataset *ds, size_t first, size_t rounds_at_entry, int rc);

// ---------------------------------------------------------------------------------- the batch pipeline
struct InflatedExt { uint64_t off, size; };      // where a file's inflated bytes lie in a batch's output
// RESIDENT form: the BAM headers of the batch's files, read from their leading blocks by the host decoder (per file of the batch)
struct ResidentBatch { std::vector<BamHeader> hdr; std::vector<uint64_t> rec_off; };
// files [f0, f1) are inflated: file f0 + k at out + ext[k].off -- or, dev_valid, the same bytes at ctx->dev_out + ext[k].off (resident: out = NULL then)
using FeedConsume = std::function<int(int f0, int f1, const uint8_t *out, const std::vector<InflatedExt> &ext, bool dev_valid)>;
// counters (optional): [0] blocks, [1] blocks inflated on the host after all, [2] kernel microseconds, [3] inflated bytes
int bgzf_read_files_device(msnv_ctx *ctx, const char *const *paths, int n, int threads, const FeedConsume &consume, uint64_t counters[4], ResidentBatch *res = nullptr);
void feed_mark(const char *what);                // MSNV_FEED_TRACE=1: wall milliseconds between the steps of the device feed, on stderr
bool want_device_inflate(msnv_ctx *ctx, const char *const *paths, int n, int threads, bool resident = false);

// The record streams of files [f0, f1) of a resident batch (headers checked against the dataset's): stream k at base + ext[k].off + rb.rec_off[k]
int resident_streams(const msnv_dataset &ds, const char *const *paths, int f0, int f1, const ResidentBatch &rb, const std::vector<InflatedExt> &ext,
                     const uint8_t *base, std::vector<const uint8_t *> &ptrs, std::vector<uint64_t> &sizes);
// The N-rank entry points take ONE batch of the device inflate: MSNV_EIO for a file that cannot be sized, MSNV_EDOMAIN when the files do not fit
int fits_one_batch(const char *who, const char *const *paths, int n);
// BAM files -> samples with the per-read stage on the device (msnv_dataset_add_sample_bams when the dataset packs on the device)
int add_bams_device_pack(msnv_dataset *ds, const char *const *bam_paths, int n, int nthreads);

}  // namespace msnv
