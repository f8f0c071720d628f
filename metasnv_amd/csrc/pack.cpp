// metasnv_amd/csrc/pack.cpp -- host side of the boundary: BAM records -> packed read columns
// (dataset.h); the tile index and the upload are finalize.cpp's.  This is the "decoded on the host ... streamed to the device
// as packed per-read columns" stage of the north star; no pileup arithmetic happens here, only
// the read-level filters that `samtools mpileup` applies before its pileup engine
// (bam_plcmd.c mplp_func, restated in SURVEY.md Appendix C) and qaCompute's read filter
// (qaCompute.cpp:461-526), both reduced to two bits per read.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <unordered_map>

#include "device.h"
#include "devpack.h"

namespace msnv {

// Piece alignment in the seq column (bytes; the qual column is twice that): dataset.h SEQ_ALIGN, 2 bytes since round 3 (round 1,
// 16 bases per lane: 16 -> 0.725 ms, 8 -> 0.665, 4 -> 0.664, 2 -> 0.651; round 3, 32 bases per lane: 8 -> 0.573, 4 -> 0.548, 2 -> 0.547).
// The compact headers store seq offsets in SEQ_ALIGN units.
constexpr uint32_t seq_align = SEQ_ALIGN;

static inline bool consumes_ref(uint32_t t) { return t == C_M || t == C_D || t == C_N || t == C_EQ || t == C_X; }
static inline bool consumes_query(uint32_t t) { return t == C_M || t == C_I || t == C_S || t == C_EQ || t == C_X; }

// qaCompute's per-read bookkeeping (qaCompute.cpp:461-473 unmapped, :518-526 MAPQ / duplicate filter): the "Other" block of
// OUT counts every record of the BAM, whatever shard it belongs to.  Returns false for reads qaCompute skips as unmapped;
// cov_ok = the read enters the coverage difference array.
static inline bool read_stats(const RecView &r, int cov_min_mapq, msnv_sample_stats &st, bool &cov_ok) {
    cov_ok = false;
    st.total_reads++;
    if ((r.flag & BAM_FUNMAP) || r.tid < 0) { st.unmapped++; return false; }
    st.any_mapped = 1;
    if (r.mapq >= cov_min_mapq) {
        if (r.flag & BAM_FPROPER_PAIR) st.proper_pairs++;
        if (r.flag & BAM_FDUP) st.duplicates++; else cov_ok = true;
    } else st.zero_quality++;
    return true;
}

// Multi-GPU decode sharding (msnv.h: msnv_records_partition): one walk over a sample's record stream that deals the
// mapped records to the rank owning their contig (order preserved inside a part) and counts qaCompute's statistics.
int records_partition(const uint8_t *rec, uint64_t n_bytes, const int32_t *owner, int n_contigs, int n_parts, int cov_min_mapq,
                      uint8_t *out, uint64_t *part_bytes, msnv_sample_stats &st) {
    std::vector<uint64_t> size((size_t)n_parts, 0);
    st = msnv_sample_stats{};
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint64_t> cur((size_t)n_parts, 0);
        if (pass == 1) { uint64_t o = 0; for (int k = 0; k < n_parts; ++k) { cur[(size_t)k] = o; o += size[(size_t)k]; } }
        uint64_t off = 0;
        while (off < n_bytes) {
            RecView r;
            if (!rec_parse(rec + off, n_bytes - off, r)) return fail(MSNV_EFORMAT, "malformed BAM record at byte %llu", (unsigned long long)off);
            const uint8_t *src = rec + off;
            off += r.size;
            if (pass == 0) {
                bool cov_ok;
                if (!read_stats(r, cov_min_mapq, st, cov_ok)) continue;
                if (r.tid >= n_contigs) return fail(MSNV_EFORMAT, "record refers to contig %d but the header has %d", r.tid, n_contigs);
            } else if ((r.flag & BAM_FUNMAP) || r.tid < 0) continue;
            const int32_t k = owner[r.tid];
            if (k < 0) continue;                                  // contig outside every shard (BED split)
            if (k >= n_parts) return fail(MSNV_EINVAL, "contig %d is owned by part %d of %d", r.tid, k, n_parts);
            if (pass == 0) size[(size_t)k] += r.size;
            else { memcpy(out + cur[(size_t)k], src, r.size); cur[(size_t)k] += r.size; }
        }
    }
    for (int k = 0; k < n_parts; ++k) part_bytes[k] = size[(size_t)k];
    return MSNV_OK;
}

// ---------------------------------------------------------------------------------- overlapping mates
// `samtools mpileup` without -x (metaSNV.py:160-165) lets htslib's pileup engine edit the base qualities of proper-pair
// mates that overlap on the reference before the -Q cutoff sees them (sam.c overlap_push / tweak_overlap_quality, htslib
// >= 1.10): where both mates have an aligned base at a reference position, agreeing bases give min(200, qa + qb) to the
// mate that was pushed first and 0 to the other; disagreeing bases give 0.8 * q (truncated) to the one of higher quality
// (ties: the first) and 0 to the other.  So each template counts once per position, and snpCall's counts depend on it.
//
// The engine walks the two CIGARs with a shared reference cursor t: x = first match position of a at or after t,
// y = first match position of b at or after x, the pair is edited iff x == y, then t = y + 1.  Consequence kept here:
// behind a stretch where a has bases and b has none (deletion / skip in b), b's next base is never edited.
struct MatchCursor {           // the M/=/X bases of one alignment in reference order
    const RecView &r; int k = 0; int64_t op_ref, op_q; int64_t ref = -1, q = -1;
    explicit MatchCursor(const RecView &rv) : r(rv), op_ref(rv.pos), op_q(0) {}
    // first match base at a reference position >= target; false when the alignment has none left
    bool seek(const int64_t target) {
        for (; k < r.n_cigar; ++k) {
            const uint32_t c = ld_u32(r.cigar + 4 * k), t = c & 15u; const int64_t l = c >> 4;
            if (t == C_M || t == C_EQ || t == C_X) {
                if (target < op_ref + l) { ref = std::max(target, op_ref); q = op_q + (ref - op_ref); return true; }
                op_ref += l; op_q += l;
            } else {
                if (t == C_D || t == C_N) op_ref += l;
                if (t == C_I || t == C_S) op_q += l;
            }
        }
        return false;
    }
};

static void tweak_overlapping_mates(const RecView &a, uint8_t *qa, const RecView &b, uint8_t *qb) {
    if (a.l_seq == 0 || b.l_seq == 0) return;
    MatchCursor ca(a), cb(b);
    int64_t t = b.pos;
    while (ca.seek(t) && cb.seek(ca.ref)) {
        t = cb.ref + 1;
        if (ca.ref != cb.ref) continue;
        if (ca.q >= a.l_seq || cb.q >= b.l_seq) return;
        const uint32_t ba = (a.seq[ca.q >> 1] >> ((~ca.q & 1) << 2)) & 0xfu, bb = (b.seq[cb.q >> 1] >> ((~cb.q & 1) << 2)) & 0xfu;
        uint8_t &x = qa[ca.q], &y = qb[cb.q];
        if (ba == bb) { const int sum = (int)x + (int)y; x = (uint8_t)(sum > 200 ? 200 : sum); y = 0; }
        else if (x >= y) { x = (uint8_t)(0.8 * x); y = 0; }
        else { y = (uint8_t)(0.8 * y); x = 0; }
    }
}

// One filtered read of pass 1, kept for pass 2 (packing).
struct KeptRead { uint64_t off; int64_t endpos; uint16_t depth_here; bool pile_ok, cov_ok; uint32_t idx; };      // idx: ordinal of the record in the stream

// ---------------------------------------------------------------------------------- snpCall's token limit
// snpCall copies every tab-separated field of a pileup line through a 10000-character token (call_vC.cpp:92-111,481-483):
// a sample's base string is CUT there and the bases behind the cut are never counted (SURVEY.md Appendix A "D1").  With
// mpileup -d 8000 that takes a stack of reads starting at one position (`^]` costs two characters per read start) or
// thousands of indel suffixes, but the reference's counts are what they are.  The string itself is never built here: where
// a sample's string can reach the limit at all (upper bound kept by the caller's sweep), the characters of every element
// are counted in pileup order -- [^ mapq] base|*|<> [+n ins | -n del] [$], elements below -Q are not printed at all
// (bam_plcmd.c pileup_seq and the text loop) -- and a base whose character lies at or behind the limit gets quality 0, so
// the device leaves it out exactly like a base below the cutoff.  Nothing else of a cut element can be counted: what
// follows a base inside its element (indel suffix, $) is skipped by snpCall's parser anyway (call_vC.cpp:506-523).
static uint32_t decimal_digits(uint32_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; ++d; } return d; }

static uint32_t max_element_chars(const RecView &r) {
    uint64_t ins = 0, del = 0;
    for (int k = 0; k < r.n_cigar; ++k) {
        const uint32_t c = ld_u32(r.cigar + 4 * k), t = c & 15u;
        if (t == C_I) ins += c >> 4;                       // consecutive insertions around a P op print as one suffix
        else if (t == C_D) del = std::max<uint64_t>(del, c >> 4);
    }
    // `^` mapq, the base, `$`; behind a base that ends an aligned block: sign, up to ten digits, the inserted / deleted bases (round 6: the 11 only
    // for a read that has an indel at all -- a sample's string is "in reach" of the limit at 2 500 plain reads, not at 667)
    return (uint32_t)std::min<uint64_t>(0x7fffffffu, 4 + ((ins | del) ? 11 + std::max(ins, del) : 0));
}

// The mark of a base whose character is cut off.  (It used to be quality 0 -- "the device leaves it out like a base below the cutoff" --
// which is not below a cutoff of 0: with -Q 0 the cut bases were counted.  metaSNV never runs -Q 0; the fuzz sweep does.)  Qualities of
// 128 and more pass every cutoff just like 127 (pack_sample clamps them), so the reads the walk below can touch are clamped first and
// the mark cannot be mistaken for a stored quality.
constexpr uint8_t QUAL_CUT = 0xfe;

template <typename MutableQual>
static void apply_token_limit(const msnv_params &P, const uint8_t *rec, uint64_t n_bytes, const std::vector<KeptRead> &kept, MutableQual &mutable_qual) {
    for (const KeptRead &kr : kept) {
        if (!kr.pile_ok) continue;
        RecView r;
        rec_parse(rec + kr.off, n_bytes - kr.off, r);
        if (r.l_seq <= 0) continue;
        uint8_t *q = mutable_qual(r);
        for (int32_t j = 0; j < r.l_seq; ++j) if (q[j] > 127) q[j] = 127;
    }
    struct Act { RecView r; int64_t end; uint32_t maxc; int k; int64_t x, y; };
    std::vector<Act> act;                                   // pileup reads alive at the current position, in push (= file) order
    uint64_t bound = 0;
    const uint64_t limit = (uint64_t)P.token_limit;
    size_t next = 0;
    while (next < kept.size() && !kept[next].pile_ok) ++next;
    int32_t tid = -1; int64_t pos = 0;
    auto peek = [&](RecView &r) { rec_parse(rec + kept[next].off, n_bytes - kept[next].off, r); };
    while (next < kept.size() || !act.empty()) {
        RecView nr{};
        if (next < kept.size()) peek(nr);
        if (act.empty()) {
            if (next >= kept.size()) break;
            tid = nr.tid; pos = nr.pos;
        }
        // reads that start here
        while (next < kept.size() && nr.tid == tid && nr.pos == pos) {
            Act a{nr, kept[next].endpos, max_element_chars(nr), 0, nr.pos, 0};
            for (; a.k < nr.n_cigar; ++a.k) {               // cursor on the first reference-consuming op (sam.c resolve_cigar2)
                const uint32_t c = ld_u32(nr.cigar + 4 * a.k), t = c & 15u;
                if (consumes_ref(t)) break;
                if (t == C_I || t == C_S) a.y += c >> 4;
            }
            act.push_back(a); bound += a.maxc;
            do ++next; while (next < kept.size() && !kept[next].pile_ok);
            if (next < kept.size()) peek(nr);
        }
        if (bound >= limit) {
            uint64_t off = 0;                               // characters of this sample's base string so far
            for (Act &a : act) {
                const RecView &r = a.r;
                bool found = false;
                while (a.k < r.n_cigar) {                   // advance to the op that holds `pos`
                    const uint32_t c = ld_u32(r.cigar + 4 * a.k), t = c & 15u; const int64_t l = c >> 4;
                    if (consumes_ref(t) && pos < a.x + l) { found = true; break; }
                    if (consumes_ref(t)) a.x += l;
                    if (consumes_query(t)) a.y += l;
                    ++a.k;
                }
                if (!found) continue;
                const uint32_t c = ld_u32(r.cigar + 4 * a.k), t = c & 15u; const int64_t l = c >> 4;
                const bool is_del = !(t == C_M || t == C_EQ || t == C_X);
                const int64_t qpos = is_del ? a.y : a.y + (pos - a.x);
                int64_t indel = 0;
                if (!is_del && a.x + l - 1 == pos && a.k + 1 < r.n_cigar) {
                    const uint32_t c2 = ld_u32(r.cigar + 4 * (a.k + 1)), t2 = c2 & 15u;
                    if (t2 == C_D) indel = -(int64_t)(c2 >> 4);
                    else if (t2 == C_I) indel = c2 >> 4;
                    else if (t2 == C_P && a.k + 2 < r.n_cigar) {
                        for (int k = a.k + 2; k < r.n_cigar; ++k) {
                            const uint32_t c3 = ld_u32(r.cigar + 4 * k), t3 = c3 & 15u;
                            if (t3 == C_I) indel += c3 >> 4;
                            else if (t3 == C_D || t3 == C_M || t3 == C_N || t3 == C_EQ || t3 == C_X) break;
                        }
                    }
                }
                uint8_t *q = (r.l_seq > 0) ? mutable_qual(r) : nullptr;
                const int qv = (q && qpos < r.l_seq) ? q[qpos] : 0;
                if (qv < P.min_baseq) continue;             // not printed at all
                const bool head = pos == r.pos, tail = pos == a.end - 1;
                if (!is_del && off + (head ? 2u : 0u) >= limit && q) q[qpos] = QUAL_CUT;      // the base's own character is cut off
                const uint64_t n_indel = (uint64_t)(indel < 0 ? -indel : indel);
                off += (head ? 2u : 0u) + 1u + (indel ? 1u + decimal_digits((uint32_t)n_indel) + n_indel : 0u) + (tail ? 1u : 0u);
            }
        }
        // next position: the following one while reads are alive, else the next read's start
        ++pos;
        size_t w = 0;
        for (size_t i = 0; i < act.size(); ++i) { if (act[i].end > pos) act[w++] = act[i]; else bound -= act[i].maxc; }
        act.resize(w);
        if (bound < limit) {                                // nothing to count before the next read arrives
            RecView r2{};
            if (next < kept.size()) peek(r2);
            if (next >= kept.size() || r2.tid != tid) { act.clear(); bound = 0; }
            else if (r2.pos > pos) {
                pos = r2.pos;
                w = 0;
                for (size_t i = 0; i < act.size(); ++i) { if (act[i].end > pos) act[w++] = act[i]; else bound -= act[i].maxc; }
                act.resize(w);
            }
        }
    }
}

struct NameKey {
    const uint8_t *p; uint32_t n;
    bool operator==(const NameKey &o) const { return n == o.n && memcmp(p, o.p, n) == 0; }
};
struct NameHash {
    size_t operator()(const NameKey &k) const { uint64_t h = 1469598103934665603ull; for (uint32_t i = 0; i < k.n; ++i) { h ^= k.p[i]; h *= 1099511628211ull; } return (size_t)h; }
};

// Pass 1 of packing a sample: the read-level filters of both tools and everything that edits base qualities BEFORE the
// pileup is counted (the overlapping-mate tweak, the token limit), on a private copy of the record stream (`patched`,
// left empty when nothing was edited).  kept: the reads pass 2 packs, in file order.
static int filter_and_edit(const msnv_dataset &ds, const uint8_t *rec, uint64_t n_bytes, msnv_sample_stats &st,
                           std::vector<KeptRead> &kept, std::vector<uint8_t> &patched, bool *cut_marks = nullptr, uint32_t *n_records = nullptr) {
    const msnv_params &P = ds.params;
    if (cut_marks) *cut_marks = false;
    const int n_contigs = (int)ds.names.size();
    uint64_t off = 0;
    int32_t last_tid = -1, last_pos = -1;
    // depth cap (mpileup -d): live pileup reads of this sample, by reference end
    typedef std::pair<int64_t, uint32_t> LiveRead;                  // {reference end, upper bound of its pileup element's characters}
    std::priority_queue<LiveRead, std::vector<LiveRead>, std::greater<LiveRead>> live;
    uint64_t live_chars = 0;                                        // upper bound of this sample's base-string length at the current position
    bool token_limit_in_reach = false;
    int32_t cap_tid = -1, cap_pos = -1; int nth_at_pos = 0; bool first_push_done = false;
    auto mutable_qual = [&](const RecView &r) -> uint8_t * {
        if (patched.empty()) patched.assign(rec, rec + n_bytes);
        return patched.data() + (r.qual - rec);
    };
    // qname -> the mate that was pushed first and still waits for its partner (htslib's overlap hash).  An entry is
    // visible while its read is alive in the pileup (end > start of the read being pushed); htslib drops it a few pushes
    // later, which can only matter for templates with three or more alignments in the file.
    struct Waiting { uint64_t off; int32_t tid; int64_t end; };
    std::unordered_map<NameKey, Waiting, NameHash> waiting;
    size_t waiting_sweep_at = 8192;

    uint32_t rec_idx = 0xffffffffu;
    while (off < n_bytes) {
        RecView r;
        if (!rec_parse(rec + off, n_bytes - off, r)) return fail(MSNV_EFORMAT, "malformed BAM record at byte %llu", (unsigned long long)off);
        const uint64_t rec_off = off;
        off += r.size;
        ++rec_idx;
        bool cov_ok = false;
        if (!read_stats(r, P.cov_min_mapq, st, cov_ok)) continue;                // unmapped (qaCompute.cpp:461-473)
        if (r.tid >= n_contigs) return fail(MSNV_EFORMAT, "record refers to contig %d but the header has %d", r.tid, n_contigs);
        if (r.tid < last_tid || (r.tid == last_tid && r.pos < last_pos)) return fail(MSNV_EFORMAT, "BAM is not coordinate sorted");
        last_tid = r.tid; last_pos = r.pos;
        if (!ds.sel[(size_t)r.tid]) continue;     // not this shard's contig

        // ---- CIGAR geometry
        int64_t rlen = 0, qlen = 0;
        bool has_ref_op = false;
        for (int k = 0; k < r.n_cigar; ++k) {
            uint32_t c = ld_u32(r.cigar + 4 * k), t = c & 15u, l = c >> 4;
            if (consumes_ref(t)) { rlen += l; has_ref_op = true; }
            if (consumes_query(t)) qlen += l;
        }
        const int64_t endpos = r.pos + (rlen ? rlen : 1);                        // bam_endpos

        // ---- mpileup read-level filters (bam_plcmd.c mplp_func order)
        bool pile_ok = !(r.flag & P.flag_filter);
        if (pile_ok && ds.has_bed) pile_ok = ds.bed_beg[(size_t)r.tid] < endpos && r.pos < ds.bed_end[(size_t)r.tid];
        if (pile_ok && ds.has_seq[(size_t)r.tid] && (int64_t)ds.seqs[(size_t)r.tid].size() <= r.pos) pile_ok = false;
        if (pile_ok && r.mapq < P.min_mapq) pile_ok = false;
        if (pile_ok && !P.count_orphans && (r.flag & BAM_FPAIRED) && !(r.flag & BAM_FPROPER_PAIR)) pile_ok = false;
        if (pile_ok && !has_ref_op) pile_ok = false;
        if (pile_ok && r.l_seq > 0 && qlen != r.l_seq)
            return fail(MSNV_EFORMAT, "CIGAR consumes %lld query bases but the read has %d", (long long)qlen, r.l_seq);
        if (pile_ok) {
            // depth cap, sam.c bam_plp_push (sample-local restatement)
            while (!live.empty() && live.top().first <= r.pos) { live_chars -= live.top().second; live.pop(); }
            if (cap_tid != r.tid) { while (!live.empty()) live.pop(); live_chars = 0; }
            if (cap_tid != r.tid || cap_pos != r.pos) { cap_tid = r.tid; cap_pos = r.pos; nth_at_pos = 0; }
            bool capped = (nth_at_pos > 0 || !first_push_done) && P.max_depth > 0 && (int64_t)live.size() > (int64_t)P.max_depth;
            first_push_done = true; ++nth_at_pos;
            if (capped) {
                pile_ok = false;
                if (!P.ignore_overlaps) waiting.erase(NameKey{r.qname, r.l_name});     // overlap_remove of a capped read
            } else {
                const uint32_t mc = max_element_chars(r);
                live.push(LiveRead{endpos, mc});
                live_chars += mc;
                if (P.token_limit > 0 && live_chars >= (uint64_t)P.token_limit) token_limit_in_reach = true;
            }
        }
        const uint16_t depth_here = (uint16_t)std::min<size_t>(live.size(), 0xffff);
        if (pile_ok && !P.ignore_overlaps && !(r.flag & BAM_FMUNMAP) && (r.flag & BAM_FPROPER_PAIR) &&
            !((r.mtid >= 0 && r.tid != r.mtid) || (std::llabs((long long)r.tlen) >= 2ll * r.l_seq && r.mpos >= endpos))) {
            // sam.c overlap_push: the mate waiting under this name gets its overlap with this read edited; otherwise this
            // read waits for its mate when that one is still to come (mate position at or after this one, or unknown)
            const NameKey key{r.qname, r.l_name};
            auto it = waiting.find(key);
            if (it != waiting.end() && (it->second.tid != r.tid || it->second.end <= r.pos)) { waiting.erase(it); it = waiting.end(); }
            if (it != waiting.end()) {
                RecView a;
                rec_parse(rec + it->second.off, n_bytes - it->second.off, a);
                uint8_t *qa = mutable_qual(a), *qb = mutable_qual(r);
                tweak_overlapping_mates(a, qa, r, qb);
                waiting.erase(it);
            } else if (r.mpos >= r.pos || ((r.flag & BAM_FPAIRED) && r.mpos == -1)) {
                waiting.emplace(key, Waiting{rec_off, r.tid, endpos});
                if (waiting.size() >= waiting_sweep_at) {                      // drop the entries no later read can see
                    for (auto w = waiting.begin(); w != waiting.end();) w = (w->second.tid != r.tid || w->second.end <= r.pos) ? waiting.erase(w) : std::next(w);
                    waiting_sweep_at = std::max<size_t>(8192, 2 * waiting.size());
                }
            }
        }
        if (!pile_ok && !cov_ok) continue;
        kept.push_back(KeptRead{rec_off, endpos, depth_here, pile_ok, cov_ok, rec_idx});
    }
    if (n_records) *n_records = rec_idx + 1u;
    if (token_limit_in_reach) { apply_token_limit(P, rec, n_bytes, kept, mutable_qual); if (cut_marks) *cut_marks = true; }
    return MSNV_OK;
}

// The record stream with the base qualities as the pileup engine sees them (msnv.h: msnv_dataset_pileup_qualities).
int pileup_qualities(const msnv_dataset &ds, const uint8_t *rec, uint64_t n_bytes, uint8_t *out) {
    msnv_sample_stats st{};
    std::vector<KeptRead> kept;
    std::vector<uint8_t> patched;
    bool cut_marks = false;
    if (int rc = filter_and_edit(ds, rec, n_bytes, st, kept, patched, &cut_marks)) return rc;
    if (n_bytes) memcpy(out, patched.empty() ? rec : patched.data(), n_bytes);
    if (cut_marks) {                              // the documented form of a cut base is quality 0 (msnv.h)
        for (const KeptRead &kr : kept) {
            RecView r;
            rec_parse(rec + kr.off, n_bytes - kr.off, r);
            uint8_t *q = out + (r.qual - rec);
            for (int32_t j = 0; j < r.l_seq; ++j) if (q[j] == QUAL_CUT) q[j] = 0;
        }
    }
    return MSNV_OK;
}

// The sequential edits for the device pack (devpack.hip): verdict per record + edited qualities.
int host_prepass(const msnv_dataset &ds, const uint8_t *rec, uint64_t n_bytes, std::vector<uint32_t> &ovr, std::vector<uint8_t> &patched, bool &cut_marks) {
    HostTimerScope ts(HT_PACK);
    msnv_sample_stats st{};
    std::vector<KeptRead> kept;
    uint32_t n_records = 0;
    cut_marks = false;
    if (int rc = filter_and_edit(ds, rec, n_bytes, st, kept, patched, &cut_marks, &n_records)) return rc;
    ovr.assign(n_records, 1u);
    for (const KeptRead &kr : kept) ovr[kr.idx] = 1u | (kr.pile_ok ? 2u : 0u) | (kr.cov_ok ? 4u : 0u) | (uint32_t)kr.depth_here << 16;
    return MSNV_OK;
}

// Packs one sample.  `ds` supplies contig selection, BED and parameters.
int pack_sample(const msnv_dataset &ds, const uint8_t *rec, uint64_t n_bytes, SampleCols &sc) {
    HostTimerScope ts(HT_PACK);
    const int n_contigs = (int)ds.names.size();
    std::vector<KeptRead> kept;
    std::vector<uint8_t> patched;                 // copy of the record stream with edited qualities (empty: nothing was edited)
    bool cut_marks = false;                       // the stream carries QUAL_CUT marks (snpCall's token limit was in reach)
    if (int rc = filter_and_edit(ds, rec, n_bytes, sc.st, kept, patched, &cut_marks)) return rc;
    const uint8_t *qual_base = patched.empty() ? rec : patched.data();          // qualities as the pileup sees them

    for (const KeptRead &kr : kept) {
        RecView r;
        rec_parse(rec + kr.off, n_bytes - kr.off, r);
        const bool pile_ok = kr.pile_ok, cov_ok = kr.cov_ok;
        const int64_t endpos = kr.endpos;
        const uint16_t depth_here = kr.depth_here;
        const uint8_t *r_qual = qual_base + (r.qual - rec);
        int64_t m_bases = 0;
        for (int k = 0; k < r.n_cigar; ++k) {
            const uint32_t c = ld_u32(r.cigar + 4 * k), t = c & 15u;
            if (t == C_M || t == C_EQ || t == C_X) m_bases += c >> 4;
        }

        if (cov_ok) {
            // qaCompute's M intervals in its own index space (qaCompute.cpp:530-552): index = pos + 1, a leading
            // S/H op is skipped without advancing, every other non-M op advances the cursor
            int64_t pp = (int64_t)r.pos + 1;
            int k = 0;
            if (r.n_cigar > 0) { const uint32_t t = ld_u32(r.cigar) & 15u; if (t == C_S || t == C_H) k = 1; }
            for (; k < r.n_cigar; ++k) {
                const uint32_t c = ld_u32(r.cigar + 4 * k), t = c & 15u, l = c >> 4;
                if (t == C_M && ds.sel[(size_t)r.tid]) {
                    // qaCompute.cpp:542-549: `++entireChr[pp]`, then `--entireChr[min(pp + l, chrSize - 1)]`.  With pp >= chrSize
                    // (a read whose cursor -- pos + 1, advanced by EVERY earlier op -- reaches the contig end; pp == chrSize is still
                    // inside the chrSize + 1 slots, beyond that the reference writes out of bounds) only the decrement at
                    // chrSize - 1 lands in the scanned range, and that position can never be covered (every read that reaches it is
                    // clamped onto it), so its coverage goes to -1 and the reference increments coverageHist[-1]: undefined there.
                    // One such read must not take a whole metaSNV run down: the library warns once per sample and computes what
                    // the reference's arithmetic says short of the out-of-bounds write -- covSum takes the -1, the position lands in
                    // no histogram bin.  Stored as the interval {L, L - 1} (begin > end) = "-1 at L - 1".
                    const int64_t L = ds.lengths[(size_t)r.tid];
                    if (pp >= L) {
                        if (!sc.warned_beyond_end) {
                            sc.warned_beyond_end = true;
                            fprintf(stderr, "msnv: warning: read at %s:%d reaches the contig end in qaCompute's index space (undefined behaviour in the reference: coverageHist[-1]); "
                                            "the last position of the contig is left out of the coverage histogram\n", ds.names[(size_t)r.tid].c_str(), r.pos + 1);
                        }
                        if (L >= 1) { sc.cov_tid.push_back(r.tid); sc.cov_beg.push_back((int32_t)L); sc.cov_end.push_back((int32_t)(L - 1)); }
                    } else { sc.cov_tid.push_back(r.tid); sc.cov_beg.push_back((int32_t)pp); sc.cov_end.push_back((int32_t)(pp + l)); }
                }
                pp += l;
            }
        }
        if (!pile_ok) continue;

        // ---- one 16-byte header per M/=/X segment piece of at most SEG_MAX bases; only aligned bases are shipped
        sc.n_pileup_bases += (uint64_t)m_bases;
        sc.n_pileup_reads++;
        // algorithmic bytes of a read = 16 B header + 4 B per CIGAR op + 4-bit bases + 1 B qualities
        // (only the aligned bases are counted; clipped / inserted bases are not shipped)
        sc.alg_8d_bytes += 16u + 4u * r.n_cigar + ((uint64_t)m_bases + 1) / 2 + (uint64_t)m_bases;
        sc.alg_cigar_bytes += 4u * r.n_cigar;
        if (sc.first_tid < 0) {
            // first pileup line of this sample (call_vC.cpp:423 drops the first line of the run)
            int64_t b = r.pos, e = endpos;
            if (ds.has_bed) { b = std::max(b, ds.bed_beg[(size_t)r.tid]); e = std::min(e, ds.bed_end[(size_t)r.tid]); }
            if (b < e) { sc.first_tid = r.tid; sc.first_beg = (int32_t)b; sc.first_end = (int32_t)e; }
        }
        // per contig: the first pileup line of an invocation that starts at this contig -- without -l, and with metaSNV's
        // split BED `name 1 LEN` (0-based [1, LEN): position 0 is excluded, metaSNV.py:92).  The driver derives the dropped
        // first line of every best_split_K file from these when all splits are written from one resident dataset.
        if (sc.first_any.empty()) { sc.first_any.assign((size_t)n_contigs, -1); sc.first_from1.assign((size_t)n_contigs, -1); }
        if (sc.first_any[(size_t)r.tid] < 0) sc.first_any[(size_t)r.tid] = r.pos;
        if (sc.first_from1[(size_t)r.tid] < 0 && endpos > 1) sc.first_from1[(size_t)r.tid] = std::max<int32_t>(r.pos, 1);
        // SEQ '*': every base prints as 'N' with quality 0 (bam_plcmd.c pileup_seq [EXT]) -- below every cutoff but -Q 0, and with -Q 0 an N
        // over a reference N is a match ('.' / ','): only then the read's pieces are shipped, as N bases of quality 0
        const bool noseq = r.l_seq == 0;
        if (noseq && ds.params.min_baseq > 0) continue;
        const std::string &refseq = ds.seqs[(size_t)r.tid];
        const bool has_ref = ds.has_seq[(size_t)r.tid];
        int64_t rp = r.pos; int64_t q = 0;
        for (int k = 0; k < r.n_cigar; ++k) {
            const uint32_t c = ld_u32(r.cigar + 4 * k), t = c & 15u, l = c >> 4;
            if (t == C_M || t == C_EQ || t == C_X) {
                for (uint32_t off = 0, n = 0; off < l; off += n) {
                    // a piece never crosses a tile boundary (contigs start on tile boundaries), so the device
                    // needs no clipping and every piece belongs to exactly one (tile, sample) pair
                    n = std::min<uint32_t>(std::min<uint32_t>(SEG_MAX, l - off), TILE - (uint32_t)((rp + off) % TILE));
                    if (sc.seq.size() > 0xffffff00ull) return fail(MSNV_EDOMAIN, "one sample holds more than 8.5 G aligned bases in this shard: shard the contigs further");
                    ReadHdr h;
                    h.gpos = (uint32_t)(rp + off);        // contig-relative until finalize
                    h.seqoff = (uint32_t)sc.seq.size();
                    h.cig = n;                            // segment length in bases
                    h.meta = META_PILEUP_OK | (uint32_t)r.mapq << 16;
                    sc.seq.resize(sc.seq.size() + (n + 1) / 2, 0xff);        // pad nibble = N
                    sc.alg_seq_bytes += (n + 1) / 2; sc.alg_qual_bytes += n;    // algorithmic bytes exclude the alignment padding
                    uint8_t *dst = sc.seq.data() + h.seqoff;
                    // BAM packs base 2i in the HIGH nibble; the device wants base j of the piece in nibble j, low first.
                    // Whole bytes at a time; a '=' base (code 0, rare) sends the piece through the per-base path below.
                    const int64_t q0 = q + off;
                    const uint8_t *src = r.seq + (q0 >> 1);
                    bool has_eq = false;
                    if (noseq) {
                        // (the bytes are N already)
                    } else if (!(q0 & 1)) {
                        for (uint32_t i = 0; i < n / 2; ++i) { const uint8_t b = src[i]; has_eq |= !(b & 0xf0u) || !(b & 0x0fu); dst[i] = (uint8_t)(b >> 4 | b << 4); }
                        if (n & 1u) { const uint8_t b = (uint8_t)(src[n / 2] >> 4); has_eq |= !b; dst[n / 2] = (uint8_t)(0xf0u | b); }
                    } else {
                        for (uint32_t i = 0; i < n / 2; ++i) { const uint8_t lo = src[i] & 0x0fu, hi = src[i + 1] & 0xf0u; has_eq |= !lo || !hi; dst[i] = (uint8_t)(lo | hi); }
                        if (n & 1u) { const uint8_t lo = src[n / 2] & 0x0fu; has_eq |= !lo; dst[n / 2] = (uint8_t)(0xf0u | lo); }
                    }
                    if (has_eq) {
                        for (uint32_t j = 0; j < n; ++j) {
                            const int64_t qq = q0 + j;
                            uint32_t code = (r.seq[qq >> 1] >> ((~qq & 1) << 2)) & 0xfu;
                            if (code == 0) {      // '=' always counts as a match (pileup_seq): ship the reference code instead
                                const int64_t g = rp + off + j;
                                code = (has_ref && g >= 0 && (size_t)g < refseq.size()) ? nt16_of_char((unsigned char)refseq[(size_t)g]) : 15u;
                                if (code == 0) code = 15u;
                            }
                            const int sh = (int)(j & 1u) * 4;
                            dst[j >> 1] = (uint8_t)((dst[j >> 1] & ~(0xf << sh)) | code << sh);  // low nibble first
                        }
                    }
                    if (has_ref && (sc.hdr.size() & 15u) == 0u) {      // one piece in 16: how noisy are these reads? (finalize_dataset: dense allele planes)
                        uint32_t mm = 0;
                        for (uint32_t j = 0; j < n; ++j) {
                            const int64_t g = rp + off + j;
                            if (g < 0 || (size_t)g >= refseq.size()) break;
                            mm += ((dst[j >> 1] >> (4u * (j & 1u))) & 0xfu) != nt16_of_char((unsigned char)refseq[(size_t)g]);
                        }
                        sc.mm_sampled_bases += n; sc.mm_sampled += mm;
                    }
                    {   // qualities above 127 (0xff = "not stored") pass every cutoff; clamping keeps the comparison
                        const size_t qs = sc.qual.size();
                        sc.qual.resize(qs + n);
                        uint8_t *qd = sc.qual.data() + qs;
                        const uint8_t *qsrc = r_qual + q0;
                        // (0x80: a base behind the token limit -- below every cutoff, pack_lowq)
                        if (noseq) for (uint32_t j = 0; j < n; ++j) qd[j] = 0;
                        else for (uint32_t j = 0; j < n; ++j) qd[j] = (cut_marks && qsrc[j] == QUAL_CUT) ? 0x80 : qsrc[j] > 127 ? 127 : qsrc[j];
                    }
                    // every piece starts on an 8-byte (seq) / 16-byte (qual) boundary
                    while (sc.seq.size() & (seq_align - 1u)) sc.seq.push_back(0xff);
                    while (sc.qual.size() < 2 * sc.seq.size()) sc.qual.push_back(0);
                    sc.hdr.push_back(h);
                    sc.tid.push_back(r.tid);
                    sc.depth.push_back(depth_here);
                    sc.end.push_back((int32_t)(rp + off + n));
                }
                rp += l; q += l;
            } else {
                if (consumes_ref(t)) rp += l;
                if (consumes_query(t)) q += l;
            }
        }
    }
    // ---- group the pieces by tile (stable: read order inside a tile); reads are sorted by start, so this
    // only moves the few pieces of reads that run into the next tile
    {
        const size_t n = sc.hdr.size();
        bool sorted = true;
        for (size_t i = 1; i < n && sorted; ++i)
            sorted = sc.tid[i - 1] < sc.tid[i] || (sc.tid[i - 1] == sc.tid[i] && sc.hdr[i - 1].gpos / TILE <= sc.hdr[i].gpos / TILE);
        if (!sorted) {
            std::vector<uint32_t> idx(n);
            for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
                if (sc.tid[x] != sc.tid[y]) return sc.tid[x] < sc.tid[y];
                return sc.hdr[x].gpos / TILE < sc.hdr[y].gpos / TILE;
            });
            std::vector<ReadHdr> h2(n); std::vector<int32_t> t2(n), e2(n); std::vector<uint16_t> d2(n);
            for (size_t i = 0; i < n; ++i) { h2[i] = sc.hdr[idx[i]]; t2[i] = sc.tid[idx[i]]; e2[i] = sc.end[idx[i]]; d2[i] = sc.depth[idx[i]]; }
            sc.hdr.swap(h2); sc.tid.swap(t2); sc.end.swap(e2); sc.depth.swap(d2);
        }
    }
    // tail padding: kernels read 16 B (qual) / 8 B (seq) chunks and may run past the last read
    for (int i = 0; i < 32; ++i) sc.seq.push_back(0xff);
    while (sc.qual.size() < 2 * sc.seq.size()) sc.qual.push_back(0);
    return MSNV_OK;
}

}  // namespace msnv
