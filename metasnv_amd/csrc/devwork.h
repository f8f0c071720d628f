// metasnv_amd/csrc/devwork.h -- what the two device stages of a dataset share on the host side of a launch (HIP only; no kernel lives here):
// devpack.hip, the per-read stage (with devscan.hip, the record scan, and devdeal.hip, the dealer: devrec.h), and devfin.hip, finalize's device side.
//   DpContig                      a contig as the kernels of both stages see it (DevPackTables::contigs)
//   ld32 .. put_piece_lane        device helpers both stages' kernels inline: unaligned loads, a piece's stored bytes, its lane's share of the columns
//   DevBuf, Timer, grid_for ...   an owned device allocation, HIP events around launches, the grid of n threads
//   pin_ensure                    the dataset's pinned block (devpack.hip), whose second half is finalize's (devfin.h: FinWords)
//   BufPool, Prim                 grow-only work buffers, rocPRIM calls over grow-only temporary storage
//   devpack_gather_pieces, devpack_emit_tail     two kernels of the round that finalize's deep-run split borrows, behind host calls
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "device.h"
#include "devpack.h"
#include "hiptry.h"

namespace msnv {

struct DpContig { long long len, seq_len, bed_beg, bed_end; unsigned long long pref_off; uint32_t sel, pad; };   // seq_len < 0: no FASTA record

// ------------------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint64_t ld64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
// seq bytes of a piece of n bases with its alignment padding (pack.cpp: pack_sample)
__device__ __host__ __forceinline__ uint32_t stored_bytes(uint32_t n) { return ((n + 1u) / 2u + SEQ_ALIGN - 1u) & ~(SEQ_ALIGN - 1u); }
// Pieces start on 4 bases, so a piece's flags start on bit 0 or 4 of a byte: whole bytes are stored, the two nibbles a piece shares with
// its neighbours' bytes are OR-ed in atomically (the flag column is cleared first).
__device__ __forceinline__ void or_byte(uint8_t *p, uint32_t v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    atomicOr(reinterpret_cast<uint32_t *>(a & ~(uintptr_t)3), v << (8u * (uint32_t)(a & 3u)));
}
__device__ __forceinline__ void store_bytes(uint8_t *p, uint64_t v, uint32_t n) {          // the n low bytes of v (n <= 8), any address
    if (n >= 8u) { __builtin_memcpy(p, &v, 8); return; }
    if (n & 4u) { const uint32_t w = (uint32_t)v; __builtin_memcpy(p, &w, 4); p += 4; v >>= 32; }
    if (n & 2u) { const uint16_t w = (uint16_t)v; __builtin_memcpy(p, &w, 2); p += 2; v >>= 16; }
    if (n & 1u) *p = (uint8_t)v;
}
// One lane's share of a piece into the columns: st stored nibbles (a multiple of 4) of lane `sub` (32 nibbles per lane), their flags in `bits`.
__device__ __forceinline__ void put_piece_lane(uint8_t *seq_col, uint8_t *qual_col, uint32_t seqoff, uint32_t sub, uint32_t sb, uint32_t st, uint64_t o0, uint64_t o1,
                                               uint32_t bits, uint32_t prev_last) {
    // ---- seq column: st / 2 bytes
    uint8_t *sp = seq_col + seqoff + 16u * sub;
    const uint32_t nb = st >> 1;
    store_bytes(sp, o0, nb < 8u ? nb : 8u);
    if (nb > 8u) store_bytes(sp + 8, o1, nb - 8u);
    // ---- flag column: bit index = nibble index of the seq column; the piece starts on bit 0 or 4 of a byte
    const unsigned long long b0 = 2ull * seqoff + 32u * sub;
    uint8_t *qp = qual_col + (b0 >> 3);
    const bool last_lane = sub == ((2u * sb - 1u) >> 5);
    const uint32_t v = st < 32u ? bits & ((1u << st) - 1u) : bits;
    if (!(b0 & 4ull)) {
        const uint32_t full = st >> 3;                                                  // whole bytes of mine
        store_bytes(qp, v, full);
        if (st & 4u) or_byte(qp + full, (v >> (8u * full)) & 0xfu);                     // a trailing nibble: the byte's other half is the next piece's (only the last lane ends on one)
    } else if (sub == 0) {
        or_byte(qp, (v & 0xfu) << 4);                                                   // the low nibble of the first byte is the previous piece's
        const uint32_t rest = st - 4u, full = rest >> 3;
        store_bytes(qp + 1, v >> 4, full);
        if ((rest & 4u) && last_lane) or_byte(qp + 1 + full, (v >> (4u + 8u * full)) & 0xfu);      // (else lane 1 writes that byte with my nibble in it)
    } else {
        const uint64_t w = (uint64_t)v << 4 | (prev_last & 0xfu);                       // the byte I start in, whole: the lane before me left its last nibble there
        const uint32_t total = st + 4u, full = total >> 3;
        store_bytes(qp, w, full);
        if ((total & 4u) && last_lane) or_byte(qp + full, (uint32_t)(w >> (8u * full)) & 0xfu);
    }
}

// ------------------------------------------------------------------------------------------ host side
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) dev_free(p); }
    int alloc(uint64_t bytes) { if (p) { dev_free(p); p = nullptr; } return dev_alloc(&p, bytes, nullptr); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    void *release() { void *q = p; p = nullptr; return q; }
};
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Timer {          // HIP events around a group of launches
    hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
    explicit Timer(hipStream_t s) : st(s) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start() { (void)hipEventRecord(a, st); }
    double stop() { (void)hipEventRecord(b, st); (void)hipEventSynchronize(b); float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return ms; }
};

inline unsigned bit_width_u64(unsigned long long v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b; }
inline dim3 grid_for(uint64_t n, uint32_t block) { return dim3((unsigned)std::max<uint64_t>(1, (n + block - 1) / block)); }

// The dataset's pinned block: at least `half` bytes in each of its two halves (devpack.hip).  The first half is the round's (DpAcc per sample),
// the second finalize's small results (devfin.h: FinWords).
int pin_ensure(msnv_dataset &ds, uint64_t half);

// Work buffers taken from a grow-only list in call order (a dataset's pool, or a caller's own list).  A failed allocation sticks: every
// later take() returns NULL and `rc` says why, so a batch of takes is followed by ONE `if (pool.rc) return pool.rc;`.
struct BufPool {
    std::vector<std::pair<void *, uint64_t>> &slots;
    size_t next = 0; int rc = MSNV_OK;
    bool exact = knob::guard_alloc();
    void *at(size_t i, uint64_t bytes) {                          // slot i, holding at least `bytes` (guarded allocations: exactly, and fresh)
        if (rc) return nullptr;
        std::pair<void *, uint64_t> &b = slots[i];
        bytes = std::max<uint64_t>(bytes, 16);
        if (b.second < bytes || (exact && b.second != bytes)) {
            if (b.first) dev_free(b.first);
            b.first = nullptr; b.second = 0;
            const uint64_t want = exact ? bytes : bytes + bytes / 8;
            if (int r = dev_alloc(&b.first, want, nullptr)) { rc = r; return nullptr; }
            b.second = want;
        }
        return b.first;
    }
    void *get(uint64_t bytes) {
        if (next >= slots.size()) slots.emplace_back(nullptr, 0);
        return at(next++, bytes);
    }
    template <typename T> T *take(uint64_t count) { return static_cast<T *>(get(count * sizeof(T))); }
    // the slots taken since mark() are handed out again after rewind(mark): in the same order, to the same uses
    size_t mark() const { return next; }
    void rewind(size_t m) { next = m; }
};

// rocPRIM calls with grow-only temporary storage: a buffer of its own (finalize), or after bind() ONE slot of a BufPool (the per-read stage:
// the slot keeps its index, so a dataset's second round allocates nothing).  Every call is rocPRIM's two -- the size query, room(), the
// launch; with `ask` it is the query alone (*ask = the larger of the two), for callers that grow the storage ONCE for several calls before
// they queue anything: a grow frees, and a free waits for the device.
struct Prim {
    hipStream_t st; DevBuf own; void *buf = nullptr; size_t cap = 0;
    BufPool *pool = nullptr; size_t slot = 0;
    explicit Prim(hipStream_t s) : st(s) {}
    int bind(BufPool &p, uint64_t bytes) {                        // the pool's next slot, `bytes` to begin with
        pool = &p; slot = p.next;
        buf = p.get(bytes);
        if (!buf) return p.rc;
        cap = (size_t)p.slots[slot].second;
        return MSNV_OK;
    }
    int room(size_t need) {
        if (need <= cap) return MSNV_OK;
        if (pool) { buf = pool->at(slot, need); if (!buf) return pool->rc; cap = (size_t)pool->slots[slot].second; }
        else { if (int rc = own.alloc(need)) return rc; buf = own.p; cap = need; }
        return MSNV_OK;
    }
    template <typename In, typename Out, typename Op> int inclusive(In in, Out out, size_t n, Op op, size_t *ask = nullptr) {
        size_t need = 0;
        HIP_TRY(rocprim::inclusive_scan(nullptr, need, in, out, n, op, st));
        if (ask) { *ask = std::max(*ask, need); return MSNV_OK; }
        if (int rc = room(need)) return rc;
        HIP_TRY(rocprim::inclusive_scan(buf, need, in, out, n, op, st));
        return MSNV_OK;
    }
    template <typename In, typename Out, typename Init, typename Op> int exclusive(In in, Out out, Init init, size_t n, Op op, size_t *ask = nullptr) {
        size_t need = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, need, in, out, init, n, op, st));
        if (ask) { *ask = std::max(*ask, need); return MSNV_OK; }
        if (int rc = room(need)) return rc;
        HIP_TRY(rocprim::exclusive_scan(buf, need, in, out, init, n, op, st));
        return MSNV_OK;
    }
    template <typename K, typename V> int sort_pairs(K *kin, K *kout, V *vin, V *vout, size_t n, unsigned end_bit, size_t *ask = nullptr) {
        size_t need = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, n, 0u, end_bit, st));
        if (ask) { *ask = std::max(*ask, need); return MSNV_OK; }
        if (int rc = room(need)) return rc;
        HIP_TRY(rocprim::radix_sort_pairs(buf, need, kin, kout, vin, vout, n, 0u, end_bit, st));
        return MSNV_OK;
    }
    // The forms most callers use, each defined out of line in ONE file, so that its rocPRIM kernels are compiled once: scan32 and sort64 in
    // devpack.hip (in front of the round), scan64 and reserve_scan32 at the top of devfin.hip.  rocPRIM's kernels enter a code object in the
    // order in which the compiler meets their first use; the templates above are instantiated wherever they are called, so devfin.hip's own
    // exclusive scan of uint32_t (the chunk cut) is in both objects.  Forms with one owner: the running maximum of the walks' ends
    // (SubWalk::scan_stops, behind which both routes reach it) and scan_sub_walk's exclusive scan over uint32_t * in devscan.hip; the sort of
    // uint32_t pairs in devdeal.hip; the scans of RecCnt and SubCnt in devpack.hip.  The scan of uint32_t into unsigned long long has two
    // users, devdeal.hip and devsub.hip (the sizes of the records a call keeps), and is in both objects.
    int scan32(const uint32_t *in, uint32_t *out, size_t n, bool inclusive_);
    int sort64(unsigned long long *kin, unsigned long long *kout, uint32_t *vin, uint32_t *vout, size_t n, unsigned end_bit);
    int scan64(const uint32_t *in, unsigned long long *out, size_t n);
    int reserve_scan32(size_t n);           // room for scans of up to n words before the first launch
};

// Two kernels of the round (devpack.hip) that finalize's deep-run split (devfin.hip: devfin_deep_runs) runs over a round it re-orders:
// the round's headers, contigs, ends and depths through a permutation (a launch, nothing else), and the 32 tail bytes of N and their flags
// behind a re-laid sample's columns (uploads its two arguments, launches, WAITS for the stream).
int devpack_gather_pieces(hipStream_t st, const uint32_t *src, const DevRound &R, ReadHdr *hdr2, int32_t *tid2, int32_t *end2, uint16_t *depth2);
int devpack_emit_tail(msnv_dataset &ds, uint8_t *seq, uint8_t *qual, unsigned long long piece_bytes);

}  // namespace msnv
