// metasnv_amd/csrc/devsub.h -- the subsampling rule of `qaCompute -a` / `samtools view -s` (qaCompute.cpp:319-325, :454-458), stated once
// for the host (subsample.cpp) and the device (devsub.hip), and the two stages that apply it to record streams.
//   A read is kept iff (wang(x31(name) ^ word) & 0xffffff) < threshold, threshold = ceil(frac * 2^24): the reference's
//   `(double)(k & 0xffffff) / 0x1000000 >= frac` drops, with integers only.  `word` is 0 for seed 0, else glibc's srand(seed); rand().
//   x31 and wang are restated from memory of htslib's khash.h (__ac_X31_hash_string, __ac_Wang_hash): DESIGN.md section 7 lists the rule as
//   unpinned against a real qaCompute or samtools.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MSNV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MSNV_HD inline
#endif

struct msnv_ctx;

namespace msnv {

// one byte of a read name into the polynomial hash: h * 31 + (signed char)c in uint32 arithmetic.  From h = 0 this is khash's form -- h = first
// byte, then every further byte up to the NUL -- since 0 * 31 + c = c; a first byte of 0 ends the name with h = 0 either way.
MSNV_HD uint32_t x31_step(uint32_t h, uint8_t c) { return h * 31u + (uint32_t)(int32_t)(int8_t)c; }
MSNV_HD uint32_t wang_hash(uint32_t k) {
    k += ~(k << 15); k ^= k >> 10; k += k << 3; k ^= k >> 6; k += ~(k << 11); k ^= k >> 16;
    return k;
}
MSNV_HD bool sub_keep_hash(uint32_t x31, uint32_t word, uint32_t threshold) { return (wang_hash(x31 ^ word) & 0xffffffu) < threshold; }

struct Subsample {                       // a dataset's setting (msnv_dataset_set_subsample); on = frac > 0
    bool on = false; uint32_t word = 0, threshold = 0; double frac = 0;
};
uint32_t sub_threshold(double frac);     // ceil(frac * 2^24), 2^24 for frac >= 1 (keeps everything), 0 for frac <= 0 or NaN
// the name of a record: its bytes up to the first NUL, at most l_name of them
uint32_t sub_x31(const uint8_t *name, uint32_t l_name);

// One stream on the host: the kept records to `out` (room for n_bytes), in order; counts = {kept, dropped}.  MSNV_EFORMAT for a malformed chain.
int records_subsample(const uint8_t *rec, uint64_t n_bytes, uint32_t word, uint32_t threshold, uint8_t *out, uint64_t *out_bytes, uint64_t counts[2]);
// Where stream i of a call lies in the device stage's output: on 16 bytes, with at least 16 readable bytes between its last possible byte and
// the next stream (the record scan reads ahead); *total = the capacity the call needs.
void sub_layout(const uint64_t *n_bytes, int n, uint64_t *out_off, uint64_t *total);
// Several streams on the device (devsub.hip): stage_streams, scan_records (n_contigs bounds the scan's guesses; INT32_MAX: unknown), one
// thread per record hashes its name (msnv_sub_measure), a scan of the kept sizes, sixteen lanes per kept record copy it (msnv_sub_copy).
int records_subsample_device(msnv_ctx *ctx, const uint8_t *const *streams, const uint64_t *n_bytes, int n, bool on_device, int n_contigs, uint32_t word, uint32_t threshold,
                             uint8_t *out, uint64_t capacity, uint64_t *out_off, uint64_t *out_bytes, uint64_t *counts, double *ms_kernel);

}  // namespace msnv
