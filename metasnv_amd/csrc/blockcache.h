// metasnv_amd/csrc/blockcache.h -- the bookkeeping of the device allocator's cache, without the device: which blocks are handed out, which
// are free, which free block serves a request and which ones go when the free ones exceed their cap.  Blocks come in and go out; no
// runtime call is made here (devmem.hip allocates, waits for the device and frees), so the policy is tested with made-up pointers
// (tests/test_blockcache.py).  Standard C++ only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace msnv {

struct CacheBlock { void *p; uint64_t bytes; int device; };

// what a request of `bytes` is allocated as, so that the next request of about its size finds the block
inline uint64_t cache_round(uint64_t bytes) {
    if (bytes <= 4096) return 4096;
    if (bytes < (1u << 20)) { uint64_t r = 4096; while (r < bytes) r <<= 1; return r; }     // powers of two below 1 MB
    return (bytes + (1u << 20) - 1) & ~(uint64_t)((1u << 20) - 1);                          // whole megabytes above
}

class BlockCache {
    mutable std::mutex mu;
    std::vector<CacheBlock> free_list;
    std::unordered_map<void *, CacheBlock> live;
    uint64_t free_total = 0;

public:
    // the smallest free block of `device` that holds at least `want` and at most 1.5 x (+ 1 MB) of it: live from now on
    bool take(int device, uint64_t want, CacheBlock *out) {
        std::lock_guard<std::mutex> lk(mu);
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < free_list.size(); ++i) {
            const CacheBlock &b = free_list[i];
            if (b.device != device || b.bytes < want || b.bytes > want + want / 2 + (1u << 20)) continue;
            if (best == SIZE_MAX || b.bytes < free_list[best].bytes) best = i;
        }
        if (best == SIZE_MAX) return false;
        *out = free_list[best];
        free_list[best] = free_list.back(); free_list.pop_back();
        free_total -= out->bytes;
        live[out->p] = *out;
        return true;
    }
    // a block the caller has just allocated
    void add_live(const CacheBlock &b) {
        std::lock_guard<std::mutex> lk(mu);
        live[b.p] = b;
    }
    // a live pointer back into its block (neither live nor free until give_back); false: not one of ours
    bool release(void *p, CacheBlock *out) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return false;
        *out = it->second;
        live.erase(it);
        return true;
    }
    // released blocks onto the free list; returns what the caller hands back to the runtime: over the cap, the largest blocks go first
    std::vector<CacheBlock> give_back(const std::vector<CacheBlock> &blocks, uint64_t cap) {
        std::vector<CacheBlock> evict;
        std::lock_guard<std::mutex> lk(mu);
        for (const CacheBlock &b : blocks) { free_list.push_back(b); free_total += b.bytes; }
        while (free_total > cap && !free_list.empty()) {
            size_t big = 0;
            for (size_t i = 1; i < free_list.size(); ++i) if (free_list[i].bytes > free_list[big].bytes) big = i;
            evict.push_back(free_list[big]); free_total -= free_list[big].bytes;
            free_list[big] = free_list.back(); free_list.pop_back();
        }
        return evict;
    }
    // every free block, for the caller to hand back
    std::vector<CacheBlock> drain() {
        std::vector<CacheBlock> out;
        std::lock_guard<std::mutex> lk(mu);
        out.swap(free_list); free_total = 0;
        return out;
    }
    // (what the tests look at)
    uint64_t free_bytes() const { std::lock_guard<std::mutex> lk(mu); return free_total; }
    std::vector<CacheBlock> free_blocks() const { std::lock_guard<std::mutex> lk(mu); return free_list; }
    bool is_live(void *p) const { std::lock_guard<std::mutex> lk(mu); return live.count(p) != 0; }
};

}  // namespace msnv
