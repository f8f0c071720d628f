// metasnv_amd/csrc/subsample.cpp -- the host half of the read subsampler (devsub.h): the seed word, the rule for one name, one stream filtered
// on a host thread (the datasets that pack on the host: MSNV_PACK=host), and the C ABI of all of it.  The device stage is devsub.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>

#include "devsub.h"
#include "msnv_internal.h"

namespace msnv {

uint32_t sub_threshold(double frac) {
    if (!(frac > 0)) return 0u;
    if (frac >= 1.0) return 1u << 24;
    return (uint32_t)std::ceil(frac * 16777216.0);                // (a power of two: the product is exact, so is the ceiling)
}

uint32_t sub_x31(const uint8_t *name, uint32_t l_name) {
    uint32_t h = 0;
    for (uint32_t i = 0; i < l_name && name[i]; ++i) h = x31_step(h, name[i]);
    return h;
}

int records_subsample(const uint8_t *rec, uint64_t n_bytes, uint32_t word, uint32_t threshold, uint8_t *out, uint64_t *out_bytes, uint64_t counts[2]) {
    uint64_t off = 0, o = 0, kept = 0, dropped = 0;
    while (off < n_bytes) {
        RecView r;
        if (!rec_parse(rec + off, n_bytes - off, r)) return fail(MSNV_EFORMAT, "malformed BAM record at byte %llu", (unsigned long long)off);
        if (sub_keep_hash(sub_x31(r.qname, r.l_name), word, threshold)) { memcpy(out + o, rec + off, r.size); o += r.size; ++kept; }
        else ++dropped;
        off += r.size;
    }
    *out_bytes = o;
    counts[0] = kept; counts[1] = dropped;
    return MSNV_OK;
}

void sub_layout(const uint64_t *n_bytes, int n, uint64_t *out_off, uint64_t *total) {
    uint64_t o = 0;
    for (int i = 0; i < n; ++i) { if (out_off) out_off[i] = o; o += (n_bytes[i] + 31) & ~15ull; }
    *total = o;
}

}  // namespace msnv

using namespace msnv;

extern "C" int msnv_subsample_seed_word(int64_t seed, uint32_t *word) {
    clear_error();
    if (!word) return fail(MSNV_EINVAL, "msnv_subsample_seed_word: NULL argument");
    if (seed < 0 || seed > 0xffffffffll) return fail(MSNV_EINVAL, "subsampling seed %lld is outside 0 .. 4294967295", (long long)seed);
    if (seed == 0) { *word = 0; return MSNV_OK; }
    // the reference's srand(seed); rand() -- libc's generator itself, whose state is the process's: one caller at a time here
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    srand((unsigned)seed);
    *word = (uint32_t)rand();
    return MSNV_OK;
}

extern "C" int msnv_subsample_keep(const char *name, uint32_t word, double frac) {
    if (!name) return 0;
    const uint32_t x = sub_x31(reinterpret_cast<const uint8_t *>(name), 0xffffffffu);
    return sub_keep_hash(x, word, sub_threshold(frac)) ? 1 : 0;
}

extern "C" int msnv_records_subsample(const uint8_t *records, uint64_t n_bytes, uint32_t word, double frac, uint8_t *out, uint64_t *out_bytes, uint64_t counts[2]) {
    clear_error();
    if (!out_bytes || !counts || (n_bytes && !records)) return fail(MSNV_EINVAL, "msnv_records_subsample: NULL argument");
    if (!(frac > 0)) { *out_bytes = n_bytes; counts[0] = counts[1] = 0; return MSNV_OK; }      // no subsampling: the stream is its own output, nothing is read or copied
    if (n_bytes && !out) return fail(MSNV_EINVAL, "msnv_records_subsample: NULL output");
    try { return records_subsample(records, n_bytes, word, sub_threshold(frac), out, out_bytes, counts); }
    catch (const std::exception &e) { return fail(MSNV_ENOMEM, "msnv_records_subsample: %s", e.what()); }
}
