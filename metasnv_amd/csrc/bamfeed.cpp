// metasnv_amd/csrc/bamfeed.cpp -- the host side of the BAM feed: BGZF files read by host threads, their blocks indexed, inflated on the
// device (inflate_k.hip) or by the host decoder, checked against their trailers and handed to a consumer batch by batch (bamfeed.h).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <thread>

#include "bamfeed.h"
#include "devpack.h"

namespace msnv {

// ---------------------------------------------------------------------------------- host threads
int pool_threads(int host_threads, int n) {
    const int t = host_threads > 0 ? host_threads : (int)msnv_default_threads();
    return std::min(t, std::max(1, n));
}

int for_each_index(size_t lo, size_t hi, int threads, size_t grain, const std::function<int(size_t)> &body,
                   const std::function<std::string(size_t)> &name_of, int timer) {
    if (hi <= lo) return MSNV_OK;
    std::atomic<size_t> next{lo};
    std::atomic<bool> failed{false};
    std::mutex mu;
    size_t bad = hi; int bad_rc = MSNV_OK; std::string bad_msg;      // the lowest failing index, under mu
    auto worker = [&]() {
        HostTimerScope ts(timer);
        for (;;) {
            const size_t i0 = next.fetch_add(grain);
            if (i0 >= hi || failed.load()) break;
            for (size_t i = i0; i < std::min(hi, i0 + grain); ++i) {
                int rc;
                try { rc = body(i); }                                  // (an exception in a worker thread would be std::terminate)
                catch (const std::exception &e) { rc = fail(MSNV_ENOMEM, "%s: %s", name_of(i).c_str(), e.what()); }
                if (!rc) continue;
                std::lock_guard<std::mutex> lock(mu);
                if (i < bad) { bad = i; bad_rc = rc; bad_msg = msnv_last_error(); }
                failed.store(true);
                break;
            }
        }
    };
    const size_t items = (hi - lo + grain - 1) / grain;
    std::vector<std::thread> th;
    for (size_t t = 0; t < std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), items)); ++t) th.emplace_back(worker);
    for (auto &t : th) t.join();
    if (!failed.load()) return MSNV_OK;
    return bad_msg.empty() ? fail(bad_rc, "%s failed", name_of(bad).c_str()) : fail(bad_rc, "%s", bad_msg.c_str());
}

// 0: *n is the file's size; 1: it cannot be opened; 2: it cannot be sized
static int size_of(const char *path, uint64_t *n) {
    FILE *f = fopen(path, "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fclose(f);
    if (sz < 0) return 2;
    *n = (uint64_t)sz;
    return 0;
}
bool file_size(const char *path, uint64_t *n) { return size_of(path, n) == 0; }
// ... for the callers that fail with it
static int file_size_or_fail(const char *path, uint64_t *n) {
    const int how = size_of(path, n);
    return !how ? MSNV_OK : fail(MSNV_EIO, how == 1 ? "cannot open %s" : "cannot stat %s", path);
}

int check_header(const msnv_dataset &ds, const BamHeader &h, const char *path) {
    if (h.names.size() != ds.names.size()) return fail(MSNV_EFORMAT, "%s: header has %zu contigs, expected %zu", path, h.names.size(), ds.names.size());
    for (size_t i = 0; i < h.names.size(); ++i)
        if (h.names[i] != ds.names[i] || h.lengths[i] != ds.lengths[i]) return fail(MSNV_EFORMAT, "%s: contig %zu differs from the first BAM's header", path, i);
    return MSNV_OK;
}

// ---------------------------------------------------------------------------------- into the device pack
// A round's streams through the subsampler (msnv_dataset_set_subsample; devsub.hip) into a device buffer of the round's own: the round then
// packs `kept` / `kept_bytes`, device-resident streams.  The buffer lives until the round has staged them (devpack_add_round copies and waits).
struct SubRound { void *buf = nullptr; std::vector<const uint8_t *> kept; std::vector<uint64_t> kept_bytes; ~SubRound() { if (buf) dev_free(buf); } };
static int subsample_round(msnv_dataset *ds, const uint8_t *const *records, const uint64_t *n_bytes, int n, bool streams_on_device, SubRound &sr) {
    std::vector<uint64_t> off((size_t)n), counts(2 * (size_t)n);
    sr.kept.assign((size_t)n, nullptr); sr.kept_bytes.assign((size_t)n, 0);
    uint64_t need = 0;
    sub_layout(n_bytes, n, nullptr, &need);
    if (int rc = dev_set_device(ds->ctx->device)) return rc;
    if (int rc = dev_alloc(&sr.buf, need + 256, nullptr)) return rc;
    if (int rc = records_subsample_device(ds->ctx, records, n_bytes, n, streams_on_device, (int)ds->names.size(), ds->sub.word, ds->sub.threshold, static_cast<uint8_t *>(sr.buf), need,
                                          off.data(), sr.kept_bytes.data(), counts.data(), nullptr)) return rc;
    for (int i = 0; i < n; ++i) sr.kept[(size_t)i] = static_cast<const uint8_t *>(sr.buf) + off[(size_t)i];
    return MSNV_OK;
}

int add_streams_device(msnv_dataset *ds, const uint8_t *const *records, const uint64_t *n_bytes, int n, bool streams_on_device, const uint8_t *in_place_base, uint64_t in_place_capacity) {
    HostTimerScope ts(HT_PACK_DEVICE_WALL);
    fin_trace_reset();
    struct Mark { ~Mark() { fin_trace("pack: whole call"); } } mark;
    const uint64_t round_bytes = knob::pack_round_bytes();
    const size_t first = ds->samples.size();
    const size_t rounds_at_entry = ds->dp.rounds.size();
    ds->samples.resize(first + (size_t)n);
    int rc = MSNV_OK;
    try {
        for (int i0 = 0; i0 < n && !rc;) {
            int i1 = i0; uint64_t b = 0;
            while (i1 < n && i1 - i0 < 2048 && (i1 == i0 || b + n_bytes[i1] <= round_bytes)) { b += n_bytes[i1]; ++i1; }
            if (ds->sub.on) {                                     // (the one flag test of a dataset that does not subsample)
                SubRound sr;
                rc = subsample_round(ds, records + i0, n_bytes + i0, i1 - i0, streams_on_device, sr);
                if (!rc) rc = devpack_add_round(*ds, first + (size_t)i0, sr.kept.data(), sr.kept_bytes.data(), i1 - i0, true);
            } else rc = devpack_add_round(*ds, first + (size_t)i0, records + i0, n_bytes + i0, i1 - i0, streams_on_device, in_place_base, in_place_capacity);
            i0 = i1;
        }
    } catch (const std::exception &e) { rc = fail(MSNV_ENOMEM, "packing on the device failed: %s", e.what()); }
    // rounds of this call that went through left their tables behind (dp.rounds, first_sample): finalize would index with them
    return rc ? fail_multi_add(ds, first, rounds_at_entry, rc) : MSNV_OK;
}

// A call that appends its samples in SEVERAL add_streams_device calls (groups of files, batches of the device inflate, groups of synthetic
// samples) and fails in a later one: the samples of the calls that went through are dropped with the rest (msnv.h: a failed add_* call adds
// nothing), and since their rounds' tables stay behind in dp.rounds the dataset is poisoned like in add_streams_device itself.
int fail_multi_add(msnv_dataset *ds, size_t first, size_t rounds_at_entry, int rc) {
    ds->samples.resize(first);
    if (ds->dp.rounds.size() != rounds_at_entry) ds->poisoned = true;
    return rc;
}

// ---------------------------------------------------------------------------------- the batch pipeline
void feed_mark(const char *what) {
    const bool on = knob::feed_trace();
    if (!on) return;
    static double last = 0;
    const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    fprintf(stderr, "[feed] %-44s %8.3f ms\n", what, last ? (now - last) * 1e3 : 0.0);
    last = now;
}

namespace {

// One batch of files [f0, f1) on its way through the stages of Feed::run.
struct Batch {
    int f0 = 0, f1 = 0;
    uint64_t ib = 0, ob = 0;                                     // compressed / inflated bytes, 16 bytes of slack behind every file
    std::vector<uint64_t> in_off;                                // per file: where its compressed bytes start
    uint8_t *in = nullptr, *out = nullptr;                       // the compressed bytes; the inflated bytes on the host (NULL: in HBM only)
    ByteBuf host_in, host_out;                                   // ... when they lie in pageable memory (resident form, host batches)
    std::vector<std::vector<BgzfBlock>> blocks; std::vector<uint64_t> total;      // per file
    std::vector<BamHeader> hdr; std::vector<uint64_t> rec_off;   // per file, resident form: read from its leading blocks
    std::vector<InfBlock> list;                                  // the blocks that have output
    std::vector<int> origin;                                     // file (of the batch) of every entry
    std::vector<uint32_t> blk_in_file;                           // ... and its index among the file's blocks (MSNV_INFLATE_CHECK counts per file)
    std::vector<InflatedExt> ext;
    bool have_list = false;
    // A batch whose staging cannot be had (pinned host memory or HBM: MSNV_ENOMEM) or whose launch fails is inflated by the host
    // decoder instead -- the call must not fail where the host path would have worked (a multi-GB BAM sizes the staging to itself)
    bool host_batch = false;
    std::vector<uint32_t> status;                                // per entry: 0 = as the device wrote it, else the host decoder's
    bool dev_valid = false;
    int rc = MSNV_OK; std::string msg;                           // of a load that ran on a thread of its own
    int nf() const { return f1 - f0; }
};

// BGZF files inflated on the device (inflate_k.hip), in two forms.
// STAGED: the files of a batch are read by `threads` host threads straight into the context's pinned staging buffer (no copy of the
// compressed bytes), their blocks are indexed there, the device inflates all blocks of the batch into the pinned output buffer, and
// consume() parses the files in place (no copy of the inflated bytes either; the buffer is reused by the next batch).  Blocks the device
// refuses are inflated by the host decoder, which words the error of a malformed file.
// RESIDENT (the device pack's): the inflated bytes never leave HBM.  The files are read into pageable memory (no pinning: a context's first
// gigabyte of pinned staging costs 0.25 s), the batch goes up as it is, every block's CRC-32 is checked by a kernel (inflate_k.hip:
// msnv_crc_blocks), only the status words come back; the BAM headers are read from the leading blocks of every file by the host decoder; a
// block the device refused or that did not check is inflated by the host decoder and patched into the device buffer.  consume() then gets
// out = nullptr and dev_valid = true.  A batch's host work is done by load_ahead, and the NEXT batch is loaded (std::async) while the
// device inflates, checks and packs the current one.
struct Feed {
    msnv_ctx *ctx; const char *const *paths; int n, threads; bool resident;
    Feed(msnv_ctx *c, const char *const *p, int n_files, int t, bool res) : ctx(c), paths(p), n(n_files), threads(t), resident(res) {}
    std::vector<uint64_t> fsize;
    uint64_t batch_in = 0;
    uint32_t check_every = 1;
    double ms = 0; uint64_t n_blocks = 0, n_host = 0, n_bytes = 0;      // counters[2], [0], [1], [3]

    int run(const FeedConsume &consume, ResidentBatch *res);
    int plan();
    void extent(Batch &b, int f0) const;
    int load(Batch &b, bool want_headers);
    std::unique_ptr<Batch> load_ahead(int f0);
    int load_staged(Batch &b, int f0);
    int list_blocks(Batch &b);
    int host_buffers(Batch &b);
    int host_takes_batch(Batch &b, const char *why);
    int staging_out(Batch &b);
    int device_buffers(Batch &b);
    int launch_staged(Batch &b) { return dev_inflate(ctx, b.ib, b.list, b.ob, b.status, &ms); }
    int launch_resident(Batch &b);
    int inflate(Batch &b, int (Feed::*launch)(Batch &));
    bool trailer_crc_ok(const Batch &b, size_t e, const uint8_t *data) const;
    bool host_block(const Batch &b, size_t e, uint8_t *dst) const;
    int bad_file(const Batch &b, int k) const;
    void check_on_host(Batch &b);
    int settle_in_hbm(Batch &b);
    int settle_on_host(Batch &b);
};

// 1. plan: the files' sizes, and the compressed bytes of a batch (tests shrink it).  1 GB (~3.6 GB inflated) where the batch goes through pinned
// staging; 2 GB for the resident form, which pins nothing: the benchmark's 160 BAMs (1.35 GB) are then ONE batch -- as two, the second one's
// files were read (page faults of fresh buffers) while the first one's 1 GB went up from pageable memory (the runtime pinning it page by
// page), and the launcher waited 90 ms for that read behind the first batch (MSNV_FEED_TRACE=1: round 5)
int Feed::plan() {
    fsize.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) if (int rc = file_size_or_fail(paths[i], &fsize[(size_t)i])) return rc;
    batch_in = knob::inflate_batch_bytes(resident);
    check_every = knob::inflate_check_every();                   // (one reading for both decoders)
    return MSNV_OK;
}
void Feed::extent(Batch &b, int f0) const {
    b.f0 = b.f1 = f0; b.ib = 0; b.in_off.clear();
    while (b.f1 < n && (b.f1 == f0 || b.ib + fsize[(size_t)b.f1] <= batch_in)) { b.in_off.push_back(b.ib); b.ib += (fsize[(size_t)b.f1] + 31) & ~15ull; ++b.f1; }   // 16 bytes of slack behind every file
}

// 2. load: the batch's files read to b.in by the host threads and their blocks indexed; want_headers: the BAM headers from the leading blocks
int Feed::load(Batch &b, bool want_headers) {
    const size_t nf = (size_t)b.nf();
    b.blocks.resize(nf); b.total.assign(nf, 0);
    if (want_headers) { b.hdr.assign(nf, BamHeader()); b.rec_off.assign(nf, 0); }
    return for_each_index(0, nf, threads, 1, [&](size_t k) -> int {
        const char *path = paths[(size_t)b.f0 + k];
        uint8_t *dst = b.in + b.in_off[k];
        const uint64_t sz = fsize[(size_t)b.f0 + k];
        {
            HostTimerScope ts(HT_READ);
            FILE *f = fopen(path, "rb");
            if (!f) return fail(MSNV_EIO, "cannot open %s", path);
            const bool whole = !sz || fread(dst, 1, sz, f) == sz;
            fclose(f);
            if (!whole) return fail(MSNV_EIO, "short read on %s", path);
        }
        memset(dst + sz, 0, 16);
        if (int rc = bgzf_index_bytes(dst, sz, path, b.blocks[k], b.total[k])) return rc;
        return want_headers ? bam_header_from_blocks(dst, b.blocks[k], path, b.hdr[k], b.rec_off[k]) : MSNV_OK;      // (leading blocks, host decoder)
    }, [&](size_t k) { return std::string(paths[(size_t)b.f0 + k]); });
}
// resident form: into pageable memory, possibly on a thread of its own (the error travels in the batch)
std::unique_ptr<Batch> Feed::load_ahead(int f0) {
    std::unique_ptr<Batch> b(new Batch());
    try {
        extent(*b, f0);
        b->rc = host_buffers(*b);
        if (!b->rc) b->rc = load(*b, true);
        if (b->rc) b->msg = msnv_last_error();
    } catch (const std::exception &e) { b->rc = MSNV_ENOMEM; b->msg = e.what(); }
    return b;
}
// staged form: into the context's pinned staging
int Feed::load_staged(Batch &b, int f0) {
    extent(b, f0);
    if (int rc = dev_inflate_staging(ctx, b.ib, 0, &b.in, &b.out)) {
        if (rc != MSNV_ENOMEM) return rc;
        b.in = b.out = nullptr;
        if (int rc2 = host_takes_batch(b, "no staging for the device inflate")) return rc2;
    }
    return load(b, false);
}

// 3. the block list: what the device inflates, where each file's output lies
int Feed::list_blocks(Batch &b) {
    b.ext.resize((size_t)b.nf());
    for (int k = 0; k < b.nf(); ++k) {
        b.ext[(size_t)k] = InflatedExt{b.ob, b.total[(size_t)k]};
        uint32_t bi = 0;
        for (const BgzfBlock &bl : b.blocks[(size_t)k]) {
            const uint32_t this_block = bi++;
            if (bl.out_size == 0) {                              // nothing for the device to write; the payload must still be an empty stream (the EOF marker is one)
                if (!bgzf_inflate_block_host(b.in + b.in_off[(size_t)k] + bl.in_off, bl.in_size, nullptr, 0)) return bad_file(b, k);
                continue;
            }
            b.list.push_back(InfBlock{b.in_off[(size_t)k] + bl.in_off, b.ob + bl.out_off, bl.in_size, bl.out_size});
            b.origin.push_back(k); b.blk_in_file.push_back(this_block);
        }
        b.ob += (b.total[(size_t)k] + 15) & ~15ull;
        n_bytes += b.total[(size_t)k];
    }
    b.have_list = true;
    return MSNV_OK;
}
int Feed::bad_file(const Batch &b, int k) const {
    return fail(MSNV_EFORMAT, "%s: BGZF inflate failed (malformed DEFLATE stream or CRC-32 mismatch)", paths[b.f0 + k]);
}

// 4. buffers.  The pageable buffers of a batch the pinned staging does not hold: its input until the files are read, its output once the
// block list says how much (a resident batch has no host copy of its output: the host decoder needs one -- round 4 wrote through a NULL
// pointer here)
int Feed::host_buffers(Batch &b) {
    if (!b.in) {
        if (!b.host_in.alloc(b.ib + 64)) return fail(MSNV_ENOMEM, "out of memory for %llu compressed bytes", (unsigned long long)b.ib);
        b.in = b.host_in.data();
    }
    if (b.have_list && !b.out) {
        if (!b.host_out.alloc(b.ob + 64)) return fail(MSNV_ENOMEM, "out of memory for %llu inflated bytes", (unsigned long long)b.ob);
        b.out = b.host_out.data();
    }
    return MSNV_OK;
}
int Feed::host_takes_batch(Batch &b, const char *why) {
    fprintf(stderr, "libmsnv: %s (%s); this batch is inflated on the host\n", why, msnv_last_error());
    clear_error();
    b.host_batch = true;
    return host_buffers(b);
}
int Feed::staging_out(Batch &b) {
    if (b.host_batch) return host_buffers(b);
    uint8_t *same_in = nullptr;
    const int rc = dev_inflate_staging(ctx, b.ib, b.ob, &same_in, &b.out);      // (the input staging does not move: it only grows when ib does)
    if (!rc || rc != MSNV_ENOMEM) return rc;
    b.out = nullptr;
    return host_takes_batch(b, "no staging for the device inflate");
}
int Feed::device_buffers(Batch &b) {
    const int rc = dev_inflate_device_buffers(ctx, b.ib, b.ob);
    feed_mark("device buffers");
    if (!rc || rc != MSNV_ENOMEM) return rc;
    return host_takes_batch(b, "no staging for the device inflate");
}

// 5. inflate
int Feed::launch_resident(Batch &b) {
    if (knob::test_resident_fail()) return fail_quiet(MSNV_ENOMEM, "resident inflate refused (MSNV_TEST_RESIDENT_FAIL)");      // (tests: the fallback to the host)
    return dev_inflate_resident(ctx, b.in, b.ib, b.list, b.blk_in_file, check_every, b.status, &ms);
}
int Feed::inflate(Batch &b, int (Feed::*launch)(Batch &)) {
    if (!b.host_batch) {
        HostTimerScope ts(HT_INFLATE_DEVICE_WALL);
        const int rc = (this->*launch)(b);
        feed_mark("upload + inflate + check");
        if (rc) {
            if (rc != MSNV_ENOMEM && rc != MSNV_EHIP) return rc;
            if (int rc2 = host_takes_batch(b, "the device inflate failed")) return rc2;
        }
    }
    if (b.host_batch) b.status.assign(b.list.size(), 1u);
    return MSNV_OK;
}

// 6. check.  Every block's output is checked against the CRC-32 of its BGZF trailer, as htslib does for the reference's tools (a block that
// does not check is handed to the host decoder like one the device refused); the host threads share the blocks.
// MSNV_INFLATE_CHECK=n: every n-th block only (0 = none: benchmarks).
bool Feed::trailer_crc_ok(const Batch &b, size_t e, const uint8_t *data) const {
    return bgzf_crc32(data, b.list[e].out_size) == ld_u32(b.in + b.list[e].in_off + b.list[e].in_size);
}
void Feed::check_on_host(Batch &b) {
    if (!check_every) return;
    (void)for_each_index(0, b.list.size(), threads, 64, [&](size_t e) -> int {
        if (!b.status[e] && !(b.blk_in_file[e] % check_every) && !trailer_crc_ok(b, e, b.out + b.list[e].out_off)) b.status[e] = 2u;
        return MSNV_OK;
    }, [](size_t) { return std::string("BGZF check"); }, HT_INFLATE_HOST);
}

// 7. settle: the blocks the device refused or that did not check go through the host decoder, whose bytes answer to the same trailer
bool Feed::host_block(const Batch &b, size_t e, uint8_t *dst) const {
    if (!bgzf_inflate_block_host(b.in + b.list[e].in_off, b.list[e].in_size, dst, b.list[e].out_size)) return false;
    return !check_every || trailer_crc_ok(b, e, dst);
}
// resident batch: the few such blocks are patched into HBM
int Feed::settle_in_hbm(Batch &b) {
    std::vector<uint8_t> tmp;
    for (size_t e = 0; e < b.list.size(); ++e) {
        if (!b.status[e]) continue;
        HostTimerScope ts(HT_INFLATE_HOST);
        ++n_host;
        tmp.resize((size_t)b.list[e].out_size + 64);
        if (!host_block(b, e, tmp.data())) return bad_file(b, b.origin[e]);
        if (int rc = dev_inflate_patch(ctx, b.list[e].out_off, tmp.data(), b.list[e].out_size)) return rc;
    }
    b.dev_valid = true;
    return MSNV_OK;
}
// ... or redone in the batch's host buffer (all of them, for a host batch), shared by the host threads
int Feed::settle_on_host(Batch &b) {
    std::atomic<uint64_t> done{0};
    int rc = MSNV_OK;
    if (b.host_batch || std::any_of(b.status.begin(), b.status.end(), [](uint32_t s) { return s != 0u; }))
        rc = for_each_index(0, b.list.size(), b.host_batch ? threads : std::min(threads, 4), 16, [&](size_t e) -> int {
            if (!b.status[e]) return MSNV_OK;
            done.fetch_add(1);
            return host_block(b, e, b.out + b.list[e].out_off) ? MSNV_OK : bad_file(b, b.origin[e]);
        }, [&](size_t e) { return std::string(paths[b.f0 + b.origin[e]]); }, HT_INFLATE_HOST);
    n_host += done.load();
    b.dev_valid = !b.host_batch && done.load() == 0;             // every block of the batch as the device wrote it: ctx->dev_out holds the same bytes as `out`
    return rc;
}

int Feed::run(const FeedConsume &consume, ResidentBatch *res) {
    feed_mark("enter");
    if (int rc = dev_set_device(ctx->device)) return rc;
    if (int rc = plan()) return rc;
    // the batch buffers in HBM go back on EVERY way out (a caller that falls back to the host path after an error must not find up to ~4.6 GB
    // of staging still attached to the context); the pinned half stays for the next call
    struct ReleaseDevice { msnv_ctx *c; ~ReleaseDevice() { dev_inflate_release_device(c); } } release_device{ctx};
    std::future<std::unique_ptr<Batch>> ahead;
    struct WaitAhead { std::future<std::unique_ptr<Batch>> &f; ~WaitAhead() { if (f.valid()) f.wait(); } } wait_ahead{ahead};      // (the loader reads this object: never leave it running)
    for (int f0 = 0; f0 < n;) {
        std::unique_ptr<Batch> held(resident ? nullptr : new Batch());
        if (resident) {
            held = ahead.valid() ? ahead.get() : load_ahead(f0);
            feed_mark("batch loaded (files read, blocks indexed)");
            if (held->rc) return fail(held->rc, "%s", held->msg.c_str());
            if (held->f1 < n) ahead = std::async(std::launch::async, &Feed::load_ahead, this, held->f1);
        } else if (int rc = load_staged(*held, f0)) return rc;
        Batch &b = *held;
        if (int rc = list_blocks(b)) return rc;
        if (resident) { res->hdr = std::move(b.hdr); res->rec_off = std::move(b.rec_off); feed_mark("block list"); }
        if (int rc = resident ? device_buffers(b) : staging_out(b)) return rc;
        if (int rc = inflate(b, resident ? &Feed::launch_resident : &Feed::launch_staged)) return rc;
        const bool in_hbm = resident && !b.host_batch;             // (checked by msnv_crc_blocks; not re-checked on the host)
        if (!in_hbm) check_on_host(b);
        if (int rc = in_hbm ? settle_in_hbm(b) : settle_on_host(b)) return rc;
        n_blocks += b.list.size();
        feed_mark("blocks settled");
        if (int rc = consume(b.f0, b.f1, b.out, b.ext, b.dev_valid)) return rc;
        feed_mark("batch consumed (statistics, pack)");
        f0 = b.f1;
    }
    return MSNV_OK;
}

}  // namespace

int bgzf_read_files_device(msnv_ctx *ctx, const char *const *paths, int n, int threads, const FeedConsume &consume, uint64_t counters[4], ResidentBatch *res) {
    Feed feed(ctx, paths, n, threads, res != nullptr);
    if (int rc = feed.run(consume, res)) return rc;
    if (counters) { counters[0] = feed.n_blocks; counters[1] = feed.n_host; counters[2] = (uint64_t)(feed.ms * 1000.0); counters[3] = feed.n_bytes; }
    return MSNV_OK;
}

// Where the BGZF blocks of a call's files are inflated: on the device when that is the faster way for THIS call.  The device path
// needs pinned staging for a batch (up to 1 GB compressed + its inflated bytes), and pinning costs ~0.25 s per GB the first time a
// context does it -- more than 32 host threads need for the whole job of the benchmark shape (160 BAMs, 1.35 GB: device path cold
// 1.5 s, host decoder 0.4 s; profiles/r03d end-to-end).  So: device when the estimated host time (compressed bytes / threads x
// ~90 MB/s per thread) exceeds the estimated device time (staging still to pin + both transfers at ~25 GB/s + a launch).
// MSNV_INFLATE=host | zlib keeps everything on the host, MSNV_INFLATE=device forces the device whatever the size.
bool want_device_inflate(msnv_ctx *ctx, const char *const *paths, int n, int threads, bool resident) {
    if (!ctx) return false;
    if (const char where = knob::inflate_where()) return where == 'd';
    uint64_t bytes = 0, largest = 0;
    for (int i = 0; i < n; ++i) {
        uint64_t z = 0;
        if (!file_size(paths[i], &z)) continue;
        bytes += z; largest = std::max(largest, z);
    }
    if (bytes < (64ull << 20)) return false;                       // the host decoder is done before the staging is set up
    const double batch_in = (double)std::max<uint64_t>(std::min<uint64_t>(bytes, 1024ull << 20), largest), batch_out = 3.6 * batch_in;
    const double to_pin = std::max(0.0, batch_in - (double)ctx->pin_in_cap) + std::max(0.0, batch_out - (double)ctx->pin_out_cap);
    // (resident: add_bams_device_pack -- nothing is pinned, the compressed bytes go up from pageable memory at ~40 GB/s, the inflated bytes stay
    // in HBM and are checked there; the kernel writes ~21 GB/s of output on a 160-BAM job: profiles/r04e_inflate_*)
    const double est_dev = resident ? (double)bytes / 40e9 + 3.6 * (double)bytes / 21e9 + 0.03 : to_pin * 0.25e-9 + (double)bytes * (1.0 + 3.6) / 25e9 + 0.02;
    const double est_host = (double)bytes / ((double)std::max(1, threads) * 90e6);
    return est_dev < est_host;
}

// ---------------------------------------------------------------------------------- the resident consumers
int resident_streams(const msnv_dataset &ds, const char *const *paths, int f0, int f1, const ResidentBatch &rb, const std::vector<InflatedExt> &ext,
                     const uint8_t *base, std::vector<const uint8_t *> &ptrs, std::vector<uint64_t> &sizes) {
    ptrs.clear(); sizes.clear();
    for (int i = f0; i < f1; ++i) {
        const size_t k = (size_t)(i - f0);
        if (int rc = check_header(ds, rb.hdr[k], paths[i])) return rc;
        if (rb.rec_off[k] > ext[k].size) return fail(MSNV_EFORMAT, "%s: truncated BAM header", paths[i]);
        ptrs.push_back(base + ext[k].off + rb.rec_off[k]);
        sizes.push_back(ext[k].size - rb.rec_off[k]);
    }
    return MSNV_OK;
}

// (against knob::inflate_batch_bytes() of the STAGED form, the 1024 MB default, although the resident pipeline these entry points run
// batches at 2048 MB: files between the two are sent the host route by the caller although they would fit.  Kept as it was.)
int fits_one_batch(const char *who, const char *const *paths, int n) {
    uint64_t ib = 0;
    for (int i = 0; i < n; ++i) {
        uint64_t z = 0;
        if (int rc = file_size_or_fail(paths[i], &z)) return rc;
        ib += (z + 31) & ~15ull;
    }
    if (n > 1 && ib > knob::inflate_batch_bytes()) return fail_quiet(MSNV_EDOMAIN, "%s: the files of the call do not fit one batch of the device inflate (%llu bytes)", who, (unsigned long long)ib);
    return MSNV_OK;
}

// BAM files -> samples with the per-read stage on the device: the files are read and inflated group by group (host threads, or the device
// inflate when the rule of want_device_inflate picks it), the record streams of a group go to HBM and are packed there (devpack.hip).
static int add_bams_resident(msnv_dataset *ds, const char *const *bam_paths, int n, int nthreads) {
    // (resident form of the pipeline: the batch's bytes exist in HBM only, its headers were read from the files' leading blocks)
    ResidentBatch rb;
    const size_t first = ds->samples.size(), rounds_at_entry = ds->dp.rounds.size();
    auto consume = [&](int f0, int f1, const uint8_t *out, const std::vector<InflatedExt> &ext, bool dev_valid) -> int {
        std::vector<const uint8_t *> ptrs; std::vector<uint64_t> sizes;
        // (a batch the host decoder had to take -- no room for it in HBM -- is in host memory: it goes up from there)
        const uint8_t *base = dev_valid ? static_cast<const uint8_t *>(ds->ctx->dev_out) : out;
        if (int rc = resident_streams(*ds, bam_paths, f0, f1, rb, ext, base, ptrs, sizes)) return rc;
        // in HBM: the records are read where the inflate kernel wrote them (no copy into a round buffer) when the batch's buffer leaves
        // the kernels' read-ahead room behind its last stream
        bool in_place = dev_valid && !(reinterpret_cast<uintptr_t>(base) & 15u) && !knob::pack_copy();
        for (size_t k = 0; k < ptrs.size() && in_place; ++k) {
            if (k > 0 && ptrs[k] < ptrs[k - 1] + sizes[k - 1]) in_place = false;
            if ((uint64_t)(ptrs[k] - base) + sizes[k] + 256 > ds->ctx->dev_out_cap) in_place = false;
        }
        return add_streams_device(ds, ptrs.data(), sizes.data(), f1 - f0, dev_valid, in_place ? base : nullptr, in_place ? ds->ctx->dev_out_cap : 0);
    };
    int rc;
    try { uint64_t cnt[4]; rc = bgzf_read_files_device(ds->ctx, bam_paths, n, nthreads, consume, cnt, &rb); }
    catch (const std::exception &e) { rc = fail(MSNV_ENOMEM, "device inflate: %s", e.what()); }
    return rc ? fail_multi_add(ds, first, rounds_at_entry, rc) : MSNV_OK;      // (a later batch failed: the earlier batches' samples go too)
}
int add_bams_device_pack(msnv_dataset *ds, const char *const *bam_paths, int n, int nthreads) {
    if (want_device_inflate(ds->ctx, bam_paths, n, nthreads, true)) return add_bams_resident(ds, bam_paths, n, nthreads);
    const size_t first = ds->samples.size(), rounds_at_entry = ds->dp.rounds.size();
    const int group = std::max(nthreads, 16);
    for (int g0 = 0; g0 < n; g0 += group) {
        const int g1 = std::min(n, g0 + group);
        std::vector<ByteBuf> bufs((size_t)(g1 - g0));
        std::vector<uint64_t> rec_off((size_t)(g1 - g0), 0);
        int rc = for_each_index((size_t)g0, (size_t)g1, nthreads, 1, [&](size_t i) -> int {
            BamHeader h;
            if (int r = bam_read(bam_paths[i], h, bufs[i - (size_t)g0], rec_off[i - (size_t)g0], 1)) return r;
            return check_header(*ds, h, bam_paths[i]);
        }, [&](size_t i) { return std::string(bam_paths[i]); });
        if (!rc) {
            std::vector<const uint8_t *> ptrs; std::vector<uint64_t> sizes;
            for (size_t k = 0; k < bufs.size(); ++k) { ptrs.push_back(bufs[k].data() + rec_off[k]); sizes.push_back(bufs[k].size() - rec_off[k]); }
            rc = add_streams_device(ds, ptrs.data(), sizes.data(), g1 - g0, false);
        }
        if (rc) return fail_multi_add(ds, first, rounds_at_entry, rc);
    }
    return MSNV_OK;
}

}  // namespace msnv
