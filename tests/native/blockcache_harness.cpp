// tests/native/blockcache_harness.cpp -- the policy of the device allocator's cache (metasnv_amd/csrc/blockcache.h) on made-up pointers
// (tests/test_blockcache.py; built with g++ from that header alone, no GPU).  "blockcache_harness CASE" runs one group of checks and
// prints "ok"; a failed check prints its line and text and the exit status is 1.  After every step that changes the free list,
// free_bytes() must be the sum of the list (consistent()).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../metasnv_amd/csrc/blockcache.h"

using namespace msnv;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

constexpr uint64_t MB = 1ull << 20;
static void *ptr(uintptr_t i) { return reinterpret_cast<void *>(i * 0x1000); }      // never dereferenced

static bool consistent(const BlockCache &c) {
    uint64_t sum = 0;
    for (const CacheBlock &b : c.free_blocks()) sum += b.bytes;
    return sum == c.free_bytes();
}
// a block of `bytes` on the free list, the way the allocator gets it there: allocated (live), released, given back
static void put_free(BlockCache &c, uintptr_t i, uint64_t bytes, int device) {
    c.add_live(CacheBlock{ptr(i), bytes, device});
    CacheBlock b{};
    CHECK(c.release(ptr(i), &b));
    CHECK(c.give_back({b}, UINT64_MAX).empty());
    CHECK(consistent(c));
}
static bool is_free(const BlockCache &c, void *p) {
    for (const CacheBlock &b : c.free_blocks()) if (b.p == p) return true;
    return false;
}

static void rounding() {
    CHECK(cache_round(1) == 4096);
    CHECK(cache_round(4096) == 4096);
    CHECK(cache_round(4097) == 8192);
    CHECK(cache_round(MB - 1) == MB);
    CHECK(cache_round(MB) == MB);
    CHECK(cache_round(MB + 1) == 2 * MB);
}

static void take() {
    const uint64_t want = 4 * MB, top = want + want / 2 + MB;
    CacheBlock b{};
    { BlockCache c; put_free(c, 1, want - MB, 0); CHECK(!c.take(0, want, &b)); CHECK(c.free_blocks().size() == 1); }          // smaller than the request
    { BlockCache c; put_free(c, 1, top, 0); CHECK(c.take(0, want, &b)); CHECK(b.p == ptr(1) && b.bytes == top && b.device == 0); }      // the window's last size
    { BlockCache c; put_free(c, 1, top + 1, 0); CHECK(!c.take(0, want, &b)); CHECK(c.free_bytes() == top + 1); }              // one byte past it
    { BlockCache c; put_free(c, 1, want, 1); CHECK(!c.take(0, want, &b)); CHECK(c.take(1, want, &b)); }                      // another device's block
    for (int order = 0; order < 2; ++order) {                                                                                // of two that fit, the smaller
        BlockCache c;
        put_free(c, 1, order ? want + MB : want + 2 * MB, 0);
        put_free(c, 2, order ? want + 2 * MB : want + MB, 0);
        CHECK(c.take(0, want, &b));
        CHECK(b.bytes == want + MB);
        CHECK(c.is_live(b.p) && !is_free(c, b.p));                                                                           // taken: live, no longer free
        CHECK(c.free_blocks().size() == 1 && c.free_bytes() == want + 2 * MB && consistent(c));
    }
}

static void release() {
    BlockCache c;
    CacheBlock b{};
    CHECK(!c.release(ptr(7), &b));                                                       // never recorded: not ours
    const uint64_t bytes = cache_round(5000);
    c.add_live(CacheBlock{ptr(7), bytes, 2});
    CHECK(c.is_live(ptr(7)) && c.free_bytes() == 0);
    CHECK(c.release(ptr(7), &b));
    CHECK(b.p == ptr(7) && b.bytes == 8192 && b.device == 2);
    CHECK(!c.is_live(ptr(7)) && !is_free(c, ptr(7)));
    CHECK(!c.release(ptr(7), &b));                                                       // (a second time: not ours any more)
    CHECK(c.give_back({b}, UINT64_MAX).empty());
    const std::vector<CacheBlock> fl = c.free_blocks();
    CHECK(fl.size() == 1 && fl[0].p == ptr(7) && fl[0].bytes == 8192 && fl[0].device == 2);
    CHECK(c.free_bytes() == 8192 && consistent(c));
}

static void evict() {
    {
        BlockCache c;
        put_free(c, 1, 2 * MB, 0); put_free(c, 2, 8 * MB, 0); put_free(c, 3, 4 * MB, 0);
        // 14 MB free + 3 MB given = 17 MB over a cap of 6 MB: 8, then 4 (9 -> 5 MB), and no further
        const std::vector<CacheBlock> ev = c.give_back({CacheBlock{ptr(4), 3 * MB, 0}}, 6 * MB);
        CHECK(ev.size() == 2 && ev[0].p == ptr(2) && ev[1].p == ptr(3));
        CHECK(c.free_bytes() == 5 * MB && consistent(c));
        CHECK(is_free(c, ptr(1)) && is_free(c, ptr(4)) && !is_free(c, ptr(2)) && !is_free(c, ptr(3)));
        CHECK(c.give_back({}, 5 * MB).empty());                                           // at the cap: nothing goes
        CHECK(c.free_bytes() == 5 * MB && consistent(c));
        const std::vector<CacheBlock> ev2 = c.give_back({}, 5 * MB - 1);                  // a byte over: the largest
        CHECK(ev2.size() == 1 && ev2[0].p == ptr(4) && c.free_bytes() == 2 * MB && consistent(c));
    }
    {
        BlockCache c;                                                                     // cap 0: everything given goes, largest first
        const std::vector<CacheBlock> ev = c.give_back({CacheBlock{ptr(1), MB, 0}, CacheBlock{ptr(2), 3 * MB, 0}, CacheBlock{ptr(3), 2 * MB, 1}}, 0);
        CHECK(ev.size() == 3 && ev[0].p == ptr(2) && ev[1].p == ptr(3) && ev[2].p == ptr(1));
        CHECK(c.free_bytes() == 0 && c.free_blocks().empty());
    }
}

static void drain() {
    BlockCache c;
    put_free(c, 1, MB, 0); put_free(c, 2, 4096, 1); put_free(c, 3, 2 * MB, 0);
    c.add_live(CacheBlock{ptr(9), MB, 0});
    const std::vector<CacheBlock> out = c.drain();
    CHECK(out.size() == 3);
    int seen[4] = {0, 0, 0, 0};
    for (const CacheBlock &b : out) for (uintptr_t i = 1; i <= 3; ++i) if (b.p == ptr(i)) ++seen[i];
    CHECK(seen[1] == 1 && seen[2] == 1 && seen[3] == 1);
    CHECK(c.free_bytes() == 0 && c.free_blocks().empty() && c.drain().empty());
    CHECK(c.is_live(ptr(9)));                                                            // (what is handed out stays handed out)
}

int main(int argc, char **argv) {
    struct { const char *name; void (*run)(); } const cases[] = {{"rounding", rounding}, {"take", take}, {"release", release}, {"evict", evict}, {"drain", drain}};
    for (const auto &c : cases) {
        if (argc == 2 && !strcmp(argv[1], c.name)) {
            c.run();
            if (!failures) printf("ok\n");
            return failures ? 1 : 0;
        }
    }
    fprintf(stderr, "usage: blockcache_harness rounding|take|release|evict|drain\n");
    return 2;
}
