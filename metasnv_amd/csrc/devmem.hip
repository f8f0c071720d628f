// metasnv_amd/csrc/devmem.hip -- device memory of the library, host code only (no kernel lives here):
//   dev_set_device, dev_resident_workgroups       the current device
//   dev_alloc, dev_free, dev_free_batch, dev_cache_trim     the process-wide allocator: runtime calls around the cache of blockcache.h, or
//                                                 (MSNV_GUARD_ALLOC=1) one guarded mapping per buffer
//   dev_upload .. dev_stream_destroy              copies, fills and streams behind plain-pointer signatures, for the files g++ compiles
//   passbufs_alloc / _grow / _free, ensure_out_for_next_pass, ensure_alt, dev_free_all     the per-pass buffers of a dataset (device.h:
//                                                 PassBufs) and everything else it holds on the device
// The launches that use these buffers are in kernels.hip (struct Pass).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "blockcache.h"
#include "device.h"
#include "hiptry.h"

namespace msnv {

uint32_t dev_resident_workgroups(uint32_t per_cu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return 256u * per_cu;
    return (uint32_t)prop.multiProcessorCount * per_cu;
}

int dev_set_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MSNV_ENODEV, "no HIP device is available (this path has no CPU fallback)");
    if (device < 0 || device >= n) return fail(MSNV_ENODEV, "HIP device %d does not exist (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    return MSNV_OK;
}

// MSNV_GUARD_ALLOC=1 (debugging; tests/test_gpu_guard.py): every device buffer is mapped through the virtual-memory API so that it ENDS at
// the end of its mapping, with unmapped address space reserved behind it -- a read or write past the end of a buffer is then a GPU memory
// fault wherever the allocator would otherwise have put a neighbour (round 3: a rocprofv3 counter pass moved the neighbours and faulted).
struct GuardedAlloc { void *va; size_t reserved, mapped; hipMemGenericAllocationHandle_t handle; };
static std::mutex g_guard_mu;
static std::unordered_map<void *, GuardedAlloc> g_guarded;
// one buffer of `bytes`, ending at the end of its mapping
static int guard_map(void **p, uint64_t bytes) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = dev;
    size_t gran = 0;
    HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum));
    if (gran == 0) gran = 2u << 20;
    GuardedAlloc g{};
    g.mapped = (size_t)((bytes + gran - 1) / gran * gran);
    g.reserved = g.mapped + gran;                               // one granule behind the buffer stays unmapped
    HIP_TRY(hipMemAddressReserve(&g.va, g.reserved, gran, nullptr, 0));
    HIP_TRY(hipMemCreate(&g.handle, g.mapped, &prop, 0));
    HIP_TRY(hipMemMap(g.va, g.mapped, 0, g.handle, 0));
    hipMemAccessDesc ad = {};
    ad.location = prop.location; ad.flags = hipMemAccessFlagsProtReadWrite;
    HIP_TRY(hipMemSetAccess(g.va, g.mapped, &ad, 1));
    const size_t used = (size_t)((bytes + 15) & ~(uint64_t)15);  // (the buffers are read with 16-byte loads: keep that alignment)
    *p = static_cast<char *>(g.va) + (g.mapped - used);
    if (int fill = 0; knob::guard_fill(&fill)) { HIP_TRY(hipMemset(g.va, fill, g.mapped)); HIP_TRY(hipStreamSynchronize(nullptr)); }      // (fresh mappings are not defined to be zero: 0 or 255 tells a read of unwritten memory)
    if (knob::guard_log()) fprintf(stderr, "[guard] %p .. %p (%llu bytes; mapping %p + %zu)\n", *p, static_cast<char *>(*p) + bytes, (unsigned long long)bytes, g.va, g.mapped);
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guarded[*p] = g;
    return MSNV_OK;
}
static void guard_unmap(void *p) {
    GuardedAlloc g{};
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        auto it = g_guarded.find(p);
        if (it == g_guarded.end()) { (void)hipFree(p); return; }
        g = it->second; g_guarded.erase(it);
    }
    (void)hipDeviceSynchronize();                               // (what hipFree does by itself)
    // the address range stays reserved: a freed buffer's addresses are unmapped for good, so a stale pointer faults too.  (Handing the
    // range back -- hipMemAddressFree -- and mapping the next buffer over it gave kernels wrong bytes on this runtime, with every
    // kernel serialised and no stale pointer anywhere: profiles/r03zq notes in MEASURED.md)
    (void)hipMemUnmap(g.va, g.mapped); (void)hipMemRelease(g.handle);
}

// Device memory goes through a small caching allocator: a buffer that is given back keeps its mapping and serves the next request of about
// its size.  hipFree of the rounds' work buffers and columns was a quarter of finalize's wall time (110 us a call on average, 0.7 ms for the
// gigabyte-sized ones; a dataset's build makes ~270 of them), and every dataset of a process asks for the same sizes again.  Blocks are
// keyed by device; a request takes the smallest free block of at least its size and at most 1.5 x (+ 1 MB) of it.  Free blocks are handed
// back to the runtime when they exceed MSNV_DEV_CACHE_MB in total (default: a sixteenth of the device's memory, at most 16 GB; 0 = no cache),
// when an allocation fails (then everything cached goes and the allocation is tried again), and by dev_cache_trim() (context destroy).
// Stream order: a block is handed on only after hipDeviceSynchronize() in dev_free -- what hipFree does itself -- so no kernel of its
// previous owner is still running when the next owner's first write (possibly on another stream) arrives.
static BlockCache g_cache;                                          // (blockcache.h: the policy; the runtime calls are made here)
static uint64_t cache_cap_bytes(int dev) {                          // per device: the default is a share of THAT device's memory (the caller has made it current)
    const long long env_mb = knob::dev_cache_mb();
    if (env_mb >= 0) return (uint64_t)env_mb << 20;
    static std::mutex mu;
    static std::unordered_map<int, uint64_t> caps;
    std::lock_guard<std::mutex> lk(mu);
    auto it = caps.find(dev);
    if (it != caps.end()) return it->second;
    size_t fr = 0, tot = 0;
    const uint64_t cap = hipMemGetInfo(&fr, &tot) != hipSuccess ? (uint64_t)1 << 30 : std::min<uint64_t>((uint64_t)tot / 16, (uint64_t)16 << 30);
    caps[dev] = cap;
    return cap;
}
void dev_cache_trim() {
    for (const CacheBlock &b : g_cache.drain()) (void)hipFree(b.p);
}
// a block from the cache, or a new one of the rounded size
static int cached_alloc(void **p, uint64_t bytes) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (cache_cap_bytes(dev) == 0) { HIP_TRY(hipMalloc(p, bytes)); return MSNV_OK; }
    const uint64_t want = cache_round(bytes);
    if (CacheBlock b; g_cache.take(dev, want, &b)) { *p = b.p; return MSNV_OK; }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) { (void)hipGetLastError(); dev_cache_trim(); e = hipMalloc(p, want); }       // (the cache must never be the reason an allocation fails)
    if (e != hipSuccess) { *p = nullptr; return fail(MSNV_EHIP, "hipMalloc of %llu bytes failed: %s", (unsigned long long)want, hipGetErrorString(e)); }
    g_cache.add_live(CacheBlock{*p, want, dev});
    return MSNV_OK;
}
// The one way back: the pointers leave the live map, ONE wait for the device, their blocks join the free list, and what is then over
// the cap goes back to the runtime together with the pointers that were never ours (allocated while the cache was off).  The device
// that is waited for and whose cap counts is the current one -- or, `own_device`, the first block's.
static void cached_release(void *const *ptrs, size_t n, bool own_device) {
    std::vector<CacheBlock> ours; std::vector<void *> foreign;
    for (size_t i = 0; i < n; ++i) {
        if (!ptrs[i]) continue;
        if (CacheBlock b; g_cache.release(ptrs[i], &b)) ours.push_back(b); else foreign.push_back(ptrs[i]);
    }
    if (!own_device || !ours.empty()) {
        int cur = own_device ? ours[0].device : 0;
        (void)hipGetDevice(&cur);
        const int dev = own_device ? ours[0].device : cur;
        if (cur != dev) (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        const uint64_t cap = cache_cap_bytes(dev);
        if (cur != dev) (void)hipSetDevice(cur);
        for (const CacheBlock &e : g_cache.give_back(ours, cap)) (void)hipFree(e.p);
    }
    for (void *p : foreign) (void)hipFree(p);                       // (hipFree waits by itself)
}

int dev_alloc(void **p, uint64_t bytes, uint64_t *acct) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (int rc = knob::guard_alloc() ? guard_map(p, bytes) : cached_alloc(p, bytes)) return rc;
    if (acct) *acct += bytes;
    return MSNV_OK;
}
void dev_free(void *p) {
    if (!p) return;
    if (knob::guard_alloc()) { guard_unmap(p); return; }
    // no kernel of the old owner is running when the next owner gets the block: the BLOCK's device is the one to wait for (a dataset or a
    // context may be destroyed while another device is current)
    cached_release(&p, 1, true);
}
// Many buffers of ONE owner at once (the device pack's tables and work buffers at the end of finalize): one wait for the device, not one per buffer.
void dev_free_batch(const std::vector<void *> &ptrs) {
    if (ptrs.empty()) return;
    if (knob::guard_alloc()) { for (void *p : ptrs) dev_free(p); return; }
    cached_release(ptrs.data(), ptrs.size(), false);            // (the owner's device is current: devpack_finish / msnv_dataset_destroy set it)
}
int dev_upload(void *dst, const void *src, uint64_t bytes) {
    if (!bytes) return MSNV_OK;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MSNV_OK;
}
int dev_download(void *dst, const void *src, uint64_t bytes) { if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return MSNV_OK; }
int dev_copy_bytes(void *dst_device, const void *src, uint64_t bytes, bool src_on_device, void *stream) {
    if (!bytes) return MSNV_OK;
    HIP_TRY(hipMemcpyAsync(dst_device, src, bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MSNV_OK;
}
// hipMemset of device memory is enqueued on the null stream and returns before it has run, and the passes run on a NON-BLOCKING stream
// that the null stream does not order: without the wait below the first kernels of a pass can meet buffers that are not zero yet (fresh
// hipMalloc memory happens to be zero, so nothing showed -- until a profiler's counter pass delayed the fill kernels and the first pass
// faulted on garbage counters, and the guarded allocator's fresh mappings gave wrong counts; tests/test_gpu_guard.py)
int dev_memset(void *dst, int v, uint64_t bytes) {
    if (bytes) { HIP_TRY(hipMemset(dst, v, bytes)); HIP_TRY(hipStreamSynchronize(nullptr)); }
    return MSNV_OK;
}
// ... or on the stream the buffer's first user runs on: ordered before it, nothing to wait for
int dev_memset_async(void *dst, int v, uint64_t bytes, void *stream) {
    if (bytes) HIP_TRY(hipMemsetAsync(dst, v, bytes, (hipStream_t)stream));
    return MSNV_OK;
}
int dev_stream_wait(void *stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return MSNV_OK; }
int dev_stream_create(void **stream) { hipStream_t s; HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); *stream = s; return MSNV_OK; }
void dev_stream_destroy(void *stream) { if (stream) (void)hipStreamDestroy((hipStream_t)stream); }

// (a pointer into one of the dataset's shared allocations is not freed by itself: DeviceCols::blocks)
static bool dev_in_block(const DeviceCols &d, const void *p) {
    for (const auto &b : d.blocks) if ((const char *)p >= (const char *)b.first && (const char *)p < (const char *)b.first + b.second) return true;
    return false;
}

// ---- a set of per-pass buffers (device.h: PassBufs): the four functions below are the only place that knows its sizes and its members
// A set's bytes are part of the dataset's count for as long as the set holds them: out while one of the functions remakes buffers, back in when it leaves.
struct SetBytes { DeviceCols &d; PassBufs &b; SetBytes(DeviceCols &d_, PassBufs &b_) : d(d_), b(b_) { d.device_bytes -= b.bytes; } ~SetBytes() { d.device_bytes += b.bytes; } };
// one buffer of `elems` elements (and `tail` bytes); a buffer that is there already goes back first, with the `old_elems` it held
template <typename T> static int set_buf(PassBufs &b, T *&p, uint64_t old_elems, uint64_t elems, uint64_t tail = 0) {
    if (p) { dev_free(p); p = nullptr; b.bytes -= old_elems * sizeof(T) + tail; }
    return dev_alloc((void **)&p, elems * sizeof(T) + tail, &b.bytes);
}
// the output columns at exactly these capacities (0: none yet -- the first pass sizes them, ensure_out)
static int set_out_caps(PassBufs &b, uint64_t cap_sites, uint64_t cap_cells) {
    if (cap_sites != b.cap_out_sites) {
        if (int rc = set_buf(b, b.site_flags, b.cap_out_sites, cap_sites, 4)) return rc;      // (+4: 32-bit atomics on the byte's aligned word)
        if (int rc = set_buf(b, b.site_elig, b.cap_out_sites, cap_sites, 4)) return rc;
        b.cap_out_sites = cap_sites;
    }
    if (cap_cells != b.cap_cells) {
        if (int rc = set_buf(b, b.ncol, 4 * b.cap_cells, 4 * cap_cells, 16)) return rc;
        if (int rc = set_buf(b, b.cov_col, b.cap_cells, cap_cells, 16)) return rc;
        b.cap_cells = cap_cells;
    }
    return MSNV_OK;
}
int passbufs_alloc(DeviceCols &d, PassBufs &b, const PassBufs &caps, void *stream) {
    SetBytes count(d, b);
    const uint64_t npos = (uint64_t)d.n_tiles * TILE, nt1 = (uint64_t)d.n_tiles + 1, per64 = npos / 64 + 1;
    // what starts zeroed stays zeroed between passes: the gate kernel clears the allele totals, the individual-rule bits and the dirty
    // words it consumes, and the counter blocks alternate (the gate kernel of a pass zeroes the next one), so no pass begins with a memset
    auto zeroed = [&](auto *&p, uint64_t elems) -> int {
        if (int rc = set_buf(b, p, 0, elems)) return rc;
        return dev_memset_async(p, 0, elems * sizeof(*p), stream);
    };
    if (int rc = zeroed(b.tot, std::max<uint64_t>(1, 4 * npos))) return rc;
    if (int rc = set_buf(b, b.part, 0, d.part_bytes)) return rc;
    if (int rc = set_buf(b, b.spill, 0, std::max<uint64_t>(1, d.n_pairs) * TILE)) return rc;
    if (d.allele_planes) if (int rc = zeroed(b.aspill, (uint64_t)d.n_pairs * 4 * TILE)) return rc;      // (rows of merged pairs are never written and never read)
    b.cap_events = caps.cap_events; b.cap_overflow = caps.cap_overflow; b.cap_sites = caps.cap_sites;
    if (int rc = set_buf(b, b.events, 0, b.cap_events)) return rc;
    if (int rc = set_buf(b, b.overflow, 0, b.cap_overflow)) return rc;
    if (int rc = set_buf(b, b.sites, 0, b.cap_sites)) return rc;
    if (int rc = set_buf(b, b.unc_sites, 0, b.cap_sites)) return rc;      // the list of sites msnv_decide_sites looks at is sized like the sites
    if (int rc = set_buf(b, b.site_row, 0, per64)) return rc;             // per 64 positions (CellMap::block_row)
    if (int rc = zeroed(b.tile_dirty, (uint64_t)d.n_work + 1)) return rc;      // one word per work item (by slot)
    if (int rc = zeroed(b.counters, 2 * CNT_WORDS)) return rc;
    b.cnt_parity = 0;
    if (int rc = zeroed(b.ind4, npos / 8 + npos / 32 + 2)) return rc;
    b.unc_bits = b.ind4 + npos / 8 + 1;
    if (int rc = set_buf(b, b.site_bits, 0, per64)) return rc;
    if (int rc = set_buf(b, b.site_rank, 0, per64)) return rc;
    if (int rc = zeroed(b.tile_site_base, nt1)) return rc;
    if (int rc = zeroed(b.tile_site_cnt, nt1)) return rc;
    if (int rc = zeroed(b.tile_cell_base, nt1)) return rc;
    // whole-tile work items write their candidate records per active tile (+ one index per whole-tile item behind the lists: the tiles
    // whose candidates do not fit a list -- stage_ovf_list)
    if (d.n_fused_tiles) {
        if (int rc = dev_alloc((void **)&b.tile_stage, (uint64_t)d.n_active_tiles * sizeof(TileStage) + (uint64_t)d.n_fused_tiles * sizeof(uint32_t), &b.bytes)) return rc;
        if (int rc = dev_memset_async(b.tile_stage, 0, (uint64_t)d.n_active_tiles * sizeof(TileStage), stream)) return rc;
    }
    return set_out_caps(b, caps.cap_out_sites, caps.cap_cells);
}
int passbufs_grow(DeviceCols &d, PassBufs &b, const RunCounts &need) {
    SetBytes count(d, b);
    auto grown = [](uint32_t cap, uint32_t n) { return n <= cap ? cap : (uint32_t)std::min<uint64_t>(0x7fffffffull, (uint64_t)n + n / 4 + 1024); };
    const uint32_t ev = grown(b.cap_events, need.n_events), ov = grown(b.cap_overflow, need.n_overflow), si = grown(b.cap_sites, need.n_sites);
    if (ev != b.cap_events) { if (int rc = set_buf(b, b.events, b.cap_events, ev)) return rc; b.cap_events = ev; }
    if (ov != b.cap_overflow) { if (int rc = set_buf(b, b.overflow, b.cap_overflow, ov)) return rc; b.cap_overflow = ov; }
    if (si != b.cap_sites) {
        if (int rc = set_buf(b, b.sites, b.cap_sites, si)) return rc;
        if (int rc = set_buf(b, b.unc_sites, b.cap_sites, si)) return rc;
        b.cap_sites = si;
    }
    return MSNV_OK;
}
void passbufs_free(DeviceCols &d, PassBufs &b) {
    SetBytes count(d, b);
    void *ptrs[] = {b.tot, b.part, b.spill, b.aspill, b.events, b.overflow, b.counters, b.ind4, b.tile_dirty, b.unc_sites, b.site_row, b.site_bits, b.site_rank, b.sites,
                    b.tile_site_base, b.tile_site_cnt, b.tile_cell_base, b.ncol, b.cov_col, b.site_flags, b.site_elig, b.tile_stage};      // (unc_bits: inside ind4)
    for (void *p : ptrs) if (p && !dev_in_block(d, p)) dev_free(p);
    b = PassBufs{};
}

// the output columns of a set hold at least n_sites / n_cells (with a quarter to spare when they have to grow)
static int ensure_out(DeviceCols &d, PassBufs &b, uint64_t n_sites, uint64_t n_cells) {
    SetBytes count(d, b);
    return set_out_caps(b, n_sites > b.cap_out_sites ? std::max<uint64_t>(n_sites + n_sites / 4, 1024) : b.cap_out_sites,
                        n_cells > b.cap_cells ? (std::max<uint64_t>(n_cells + n_cells / 4, 1u << 16) + 7) & ~7ull : b.cap_cells);      // (a multiple of 8: every column starts on 16 bytes)
}
// ... before a pass: room for half as many sites and cells again as the last pass found
int ensure_out_for_next_pass(DeviceCols &d) {
    return ensure_out(d, d, std::max<uint64_t>(d.last_sites + d.last_sites / 2, 4096), std::max<uint64_t>(d.last_cells + d.last_cells / 2, 1u << 18));
}

// Second set of per-pass buffers, sized like the first (re-made when the first set was grown).  Its fills are queued on `stream` and waited
// for: the passes run on two streams that nothing else orders behind them.
int ensure_alt(DeviceCols &d, void *stream) {
    PassBufs &a = d.alt;
    if (a.tot && a.cap_events == d.cap_events && a.cap_overflow == d.cap_overflow && a.cap_sites == d.cap_sites && a.cap_out_sites == d.cap_out_sites && a.cap_cells == d.cap_cells) return MSNV_OK;
    passbufs_free(d, a);
    if (int rc = passbufs_alloc(d, a, d, stream)) return rc;
    return dev_stream_wait(stream);
}

void dev_free_all(DeviceCols &d) {
    passbufs_free(d, d); passbufs_free(d, d.alt);
    void *ptrs[] = {d.hdr, d.hdr8, d.hdr4, d.hdr8m, d.merged_groups, d.tile_pair_merged, d.blk, d.seq, d.qual, d.s_read_base, d.s_seq_base, d.ref4, d.ref_lc, d.pairs,
                    d.tile_pair_start, d.work, d.chunks, d.tile_vbeg, d.tile_vend, d.tile_slot_start, d.tile_slot_u16, d.tile_slot_wide, d.slot_off, d.gate_tiles, d.tile_nslots,
                    d.cov_iv, d.s_cov_base, d.cov_pairs, d.cov_work, d.tile_len, d.tile_contig_dev, d.cov_acc, d.tile_stage_idx, d.gate_tiles_dense, d.gate_tiles_staged, d.gather_tiles, d.active_tiles};
    for (void *p : ptrs) if (p && !dev_in_block(d, p)) dev_free(p);
    void *aptrs[] = {d.ann.seg_beg, d.ann.seg_end, d.ann.seg_gene, d.ann.genes, d.ann.contigs, d.ann.codons, d.ann.out, d.ann.err};
    for (void *p : aptrs) dev_free(p);
    for (void *e : d.timing_events) if (e) (void)hipEventDestroy((hipEvent_t)e);
    for (void *e : d.event_pool) (void)hipEventDestroy((hipEvent_t)e);
    if (d.pinned_cnt) (void)hipHostFree(d.pinned_cnt);
    for (const auto &b : d.blocks) dev_free(b.first);
    if (d.stream2) (void)hipStreamDestroy((hipStream_t)d.stream2);
    d = DeviceCols{};
}

}  // namespace msnv

extern "C" int msnv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
