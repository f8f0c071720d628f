// metasnv_amd/csrc/profile.cpp -- host side of subpopr's useGenotypesToProfileSubpops -> writeSubpopsForAllSamples (src/subpopr/R/profileSubpops.R:
// 228-274, writeSubpopsForAllSamples.R) and of useSpeciesAbundToCalcSubspeciesAbund -> writeSubpopAbundSpeciesAbund (profileSubpops.R:277-310,
// writeSubpopAbund.R:99-169).  The kernel is profile_k.hip.
//
//   msnv_subpop_profile_columns   the kernel on arrays: per column the counts and the two middle order statistics
//   msnv_subpop_profile_files     the stage: <species>_<cluster>.pos.freq and <species>_<cluster>_hap_positions.tab in, <species>_extended_clustering_*
//                                 out
//   msnv_subpop_abundance_files   <species>_extended_clustering_wFreq.tab and a species abundance table in, <species>_allClust_relativeAbund.tab and
//                                 <species>_clust_<x>_hap_coverage_extended_normed.tab out; host only (two fp64 operations per cell)
// What is on the device: every count, every prevalence's numerator and denominator, every median (the two middle order statistics; their mean is
// one r_mean of two values here) -- all of them exact, and everything a decision of the stage rests on (the keep rule, the sums, the bad samples,
// the assignment).  What is on the host: reading and writing, and the summary table's mean and standardDeviation columns, over the compact G x S
// copy that also goes to the device.  R computes them in long double (a sequential 80-bit sum, a second pass over the deviations, for sd the
// squared deviations about the mean rounded to double); an fp64 device sum cannot reproduce that bit for bit, and no guard is practical: the long
// double rule's own error bound, about G * 2^-64 relative, already reaches the 15th printed digit at real G, so a device value could not be told
// from a wrong one by a bound.  The two columns drive no decision; r_mean and r_sd (rtext.cpp) state the rule.
// Everything here is restated from reading the R code; no R was run (unpinned, with the divergences: byte order of the cluster
// files where list.files sorts by locale; a listed position the .pos.freq lacks is one all-NA row whether flipped or not; the two cases where R binds
// columns of different samples are refused; a duplicate id is refused; a single frequency column is kept a table in the abundance stage).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <dirent.h>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "dataset.h"
#include "device.h"

namespace msnv {

namespace {

// the non-empty lines of a text, without their newline and a carriage return before it
std::vector<std::string> lines_of(const std::string &text) {
    std::vector<std::string> out;
    size_t p = 0;
    while (p < text.size()) {
        size_t nl = text.find('\n', p);
        if (nl == std::string::npos) nl = text.size();
        size_t e = nl;
        if (e > p && text[e - 1] == '\r') --e;
        if (e > p) out.emplace_back(text, p, e - p);
        p = nl + 1;
    }
    return out;
}

std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out;
    size_t b = 0;
    for (size_t p = 0; p <= s.size(); ++p)
        if (p == s.size() || s[p] == sep) { out.emplace_back(s, b, p - b); b = p + 1; }
    return out;
}

inline bool parse_number(const std::string &t, double &v) { return parse_finite(t.data(), t.data() + t.size(), v); }

// contig:ann:pos:base -> contig:pos:base (writeSubpopsForAllSamples.R:57-58)
bool freq_id(const std::string &id, std::string &out) {
    const std::vector<std::string> f = split(id, ':');
    if (f.size() < 4) return false;
    out = f[0] + ":" + f[2] + ":" + f[3];
    return true;
}

// contig:ann:pos:T>A:. -> contig:pos:A; sub(".>", "", x) removes the first '>' and the character before it (:64-67)
bool hap_id(const std::string &id, std::string &out) {
    const std::vector<std::string> f = split(id, ':');
    if (f.size() < 4) return false;
    std::string base = f[3];
    const size_t gt = base.find('>', 1);
    if (gt != std::string::npos) base.erase(gt - 1, 2);
    out = f[0] + ":" + f[2] + ":" + base;
    return true;
}

struct Columns {                                                        // what the kernel returns for one matrix
    std::vector<uint32_t> called, gt0, ge5, eq0, eq100;
    std::vector<double> lo, hi;
    explicit Columns(size_t s) : called(s), gt0(s), ge5(s), eq0(s), eq100(s), lo(s), hi(s) {}
};

int profile_columns(msnv_ctx *ctx, const char *who, int64_t n_rows, int32_t S, const double *rows, const uint8_t *flip, int32_t cols_per_pass, uint32_t *called,
                    uint32_t *gt0, uint32_t *ge5, uint32_t *eq0, uint32_t *eq100, double *lo, double *hi, double *ms_kernel) {
    if (S < 1 || S > (int32_t)GENO_MAX_SAMPLES) return fail(MSNV_EDOMAIN, "%s: %d sample columns (1 to %u)", who, S, GENO_MAX_SAMPLES);
    if (n_rows < 1 || n_rows > 0x7fffffffll) return fail(MSNV_EDOMAIN, "%s: %lld rows (1 to 2147483647)", who, (long long)n_rows);
    if (cols_per_pass < 0) return fail(MSNV_EINVAL, "%s: cols_per_pass = %d", who, cols_per_pass);
    if (int rc = dev_set_device(ctx->device)) return rc;
    uint32_t *counts[5] = {called, gt0, ge5, eq0, eq100};
    bool outside = false;
    if (int rc = dev_profile_columns(rows, (uint32_t)n_rows, (uint32_t)S, flip, (uint32_t)cols_per_pass, ctx->stream, counts, lo, hi, &outside, ms_kernel)) return rc;
    if (outside) return fail(MSNV_EDOMAIN, "%s: a cell is neither NA nor within [0, 100]", who);
    return MSNV_OK;
}

struct SummaryRow { uint32_t sample; double mean, median, sd, prevalence, prevalence5; bool sd_na; uint32_t n0, n100, n_na; };

struct Cluster {
    int64_t number;
    std::vector<SummaryRow> rows;                                      // kept columns, in sample order
};

// one cluster: the G x S matrix in the order of the positions file, the kernel, the kept columns
int profile_cluster(msnv_ctx *ctx, const std::string &freq_path, const std::string &hap_path, const std::vector<std::string> &samples, double max_prop_uncalled,
                    Cluster &cl, double *ms_kernel) {
    const size_t S = samples.size();
    std::string text;
    if (int rc = slurp(freq_path, text)) return rc;
    std::unordered_map<std::string, size_t> row_of;
    std::vector<double> cells;
    uint64_t lineno = 0;
    for (const std::string &ln : lines_of(text)) {
        ++lineno;
        const std::vector<std::string> f = split(ln, '\t');
        if (f.size() != S + 1)
            return fail(MSNV_EFORMAT, "File: %s does not have expected number of columns (each column is a sample). According to all_samples, it should have %zu columns.",
                        freq_path.c_str(), S);
        std::string id;
        if (!freq_id(f[0], id)) return fail(MSNV_EFORMAT, "%s:%llu: the id '%s' is not contig:annotation:position:allele", freq_path.c_str(), (unsigned long long)lineno, f[0].c_str());
        if (!row_of.emplace(id, row_of.size()).second) return fail(MSNV_EFORMAT, "%s:%llu: the id '%s' occurs twice", freq_path.c_str(), (unsigned long long)lineno, id.c_str());
        for (size_t s = 1; s <= S; ++s) {
            double v;
            if (!parse_number(f[s], v)) return fail(MSNV_EFORMAT, "%s:%llu: '%s' is not a number", freq_path.c_str(), (unsigned long long)lineno, f[s].c_str());
            cells.push_back(v == -1.0 ? std::nan("") : v);             // makeNA
        }
    }
    text.clear();
    if (int rc = slurp(hap_path, text)) return rc;
    std::vector<size_t> src;                                            // per listed position: its row of the .pos.freq, or npos
    std::vector<uint8_t> flip;
    std::unordered_set<std::string> seen;
    lineno = 0;
    for (const std::string &ln : lines_of(text)) {
        if (++lineno == 1) {
            if (ln != "posId\tflip") return fail(MSNV_EFORMAT, "%s:1: the header is '%s', not 'posId<TAB>flip'", hap_path.c_str(), ln.c_str());
            continue;
        }
        const std::vector<std::string> f = split(ln, '\t');
        std::string id;
        if (f.size() != 3 || (f[2] != "TRUE" && f[2] != "FALSE") || !hap_id(f[1], id))
            return fail(MSNV_EFORMAT, "%s:%llu: a row is a counter, contig:annotation:position:allele and TRUE or FALSE", hap_path.c_str(), (unsigned long long)lineno);
        if (!seen.insert(id).second) return fail(MSNV_EFORMAT, "%s:%llu: the id '%s' occurs twice", hap_path.c_str(), (unsigned long long)lineno, id.c_str());
        auto it = row_of.find(id);
        src.push_back(it == row_of.end() ? std::string::npos : it->second);
        flip.push_back(f[2] == "TRUE");
    }
    const size_t G = src.size();
    if (G == 0) return MSNV_OK;                                        // nrow(data) == 0: "No data"
    std::vector<double> m(G * S, std::nan(""));
    for (size_t g = 0; g < G; ++g) if (src[g] != std::string::npos) std::copy_n(cells.data() + src[g] * S, S, m.data() + g * S);
    std::vector<double>().swap(cells);
    Columns col(S);
    if (int rc = profile_columns(ctx, freq_path.c_str(), (int64_t)G, (int32_t)S, m.data(), flip.data(), 0, col.called.data(), col.gt0.data(), col.ge5.data(), col.eq0.data(),
                                 col.eq100.data(), col.lo.data(), col.hi.data(), ms_kernel)) return rc;
    const double need = max_prop_uncalled * (double)G;
    std::vector<double> x;
    for (size_t s = 0; s < S; ++s) {
        if (!((double)col.called[s] >= need)) continue;
        x.clear();
        for (size_t g = 0; g < G; ++g) {
            const double v = m[g * S + s];
            if (v == v) x.push_back(flip[g] ? 100.0 - v : v);
        }
        const double mids[2] = {col.lo[s], col.hi[s]}, n = (double)col.called[s];
        SummaryRow r;
        r.sample = (uint32_t)s;
        r.mean = r_mean(x.data(), x.size());
        r.median = r_mean(mids, 2);
        r.sd_na = x.size() < 2;
        r.sd = r.sd_na ? 0.0 : r_sd(x.data(), x.size());
        r.prevalence = (double)col.gt0[s] / n;
        r.prevalence5 = (double)col.ge5[s] / n;
        r.n0 = col.eq0[s]; r.n100 = col.eq100[s]; r.n_na = (uint32_t)G - col.called[s];
        cl.rows.push_back(r);
    }
    return MSNV_OK;
}

// make.names for the headers read.table meets here: a name that does not start with a letter (or a dot not followed by a digit) gets an X, every
// character that is not a letter, a digit, '.' or '_' becomes '.'
std::string r_make_name(std::string n) {
    for (char &c : n) if (!isalnum((unsigned char)c) && c != '.' && c != '_') c = '.';
    const bool ok = !n.empty() && (isalpha((unsigned char)n[0]) || (n[0] == '.' && !(n.size() > 1 && isdigit((unsigned char)n[1]))));
    return ok ? n : "X" + n;
}

std::string last_three(const std::vector<std::string> &v) {
    std::string out;
    for (size_t i = v.size() > 3 ? v.size() - 3 : 0; i < v.size(); ++i) { if (!out.empty()) out += ", "; out += v[i]; }
    return out;
}

}  // namespace
}  // namespace msnv

using namespace msnv;

extern "C" int msnv_subpop_profile_columns(msnv_ctx *ctx, int64_t n_rows, int32_t n_samples, const double *rows, const uint8_t *flip, int32_t cols_per_pass,
                                           uint32_t *n_called, uint32_t *n_gt0, uint32_t *n_ge5, uint32_t *n_eq0, uint32_t *n_eq100, double *mid_lo, double *mid_hi,
                                           double *ms_kernel) {
    clear_error();
    if (ms_kernel) *ms_kernel = 0;
    if (!ctx || !rows || !flip || !n_called || !n_gt0 || !n_ge5 || !n_eq0 || !n_eq100 || !mid_lo || !mid_hi) return fail(MSNV_EINVAL, "msnv_subpop_profile_columns: NULL argument");
    return profile_columns(ctx, "msnv_subpop_profile_columns", n_rows, n_samples, rows, flip, cols_per_pass, n_called, n_gt0, n_ge5, n_eq0, n_eq100, mid_lo, mid_hi, ms_kernel);
}

extern "C" int msnv_subpop_profile_files(msnv_ctx *ctx, const char *species, const char *out_dir, const char *all_samples_path, double max_prop_uncalled,
                                         double min_genotype_abundance, int64_t result[8], double *ms_kernel) {
    clear_error();
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    if (!ctx || !species || !out_dir || !all_samples_path) return fail(MSNV_EINVAL, "msnv_subpop_profile_files: NULL argument");
    if (!(max_prop_uncalled > 0.0 && max_prop_uncalled <= 1.0)) return fail(MSNV_EDOMAIN, "msnv_subpop_profile_files: max_prop_uncalled = %g (0 < proportion <= 1)", max_prop_uncalled);
    if (min_genotype_abundance != min_genotype_abundance) return fail(MSNV_EDOMAIN, "msnv_subpop_profile_files: min_genotype_abundance is NaN");
    const std::string sp = species, dir = std::string(out_dir) + "/", prefix = dir + sp + "_extended_clustering", stat_path = prefix + "_stat.txt";

    // ---- the sample names: basenames of all_samples' lines, in file order
    std::vector<std::string> samples;
    {
        std::string text;
        if (int rc = slurp(all_samples_path, text)) return rc;
        for (const std::string &ln : lines_of(text)) {
            size_t b = 0;
            while (b < ln.size() && (ln[b] == ' ' || ln[b] == '\t')) ++b;
            size_t e = b;
            while (e < ln.size() && ln[e] != ' ' && ln[e] != '\t') ++e;
            if (e == b || ln[b] == '#') continue;
            std::string path(ln, b, e - b);
            while (path.size() > 1 && path.back() == '/') path.pop_back();
            const size_t slash = path.rfind('/');
            samples.push_back(slash == std::string::npos ? path : path.substr(slash + 1));
        }
    }
    if (samples.empty()) return fail(MSNV_EFORMAT, "%s: no sample", all_samples_path);

    // ---- <out_dir>/<species>_*.pos.freq, in byte order of their names
    std::vector<std::string> files;
    {
        DIR *d = opendir(out_dir);
        if (!d) return fail(MSNV_EIO, "Cannot open %s: %s", out_dir, strerror(errno));
        const std::string head = sp + "_", tail = ".pos.freq";
        while (struct dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() >= head.size() + tail.size() && n.compare(0, head.size(), head) == 0 && n.compare(n.size() - tail.size(), tail.size(), tail) == 0) files.push_back(n);
        }
        closedir(d);
        std::sort(files.begin(), files.end());
    }
    if (result) result[1] = (int64_t)files.size();
    const std::string none_usable = "Species " + sp + ": 0/" + std::to_string(files.size()) + " clusters had usable placing data.";
    if (files.empty()) {
        if (result) result[0] = MSNV_PROFILE_NO_FILES;
        return append_line(stat_path, none_usable);
    }

    // ---- per cluster file: the kernel and the kept samples
    std::vector<Cluster> usable;
    for (const std::string &name : files) {
        const std::string spec_hap = name.substr(0, name.find('.'));
        const size_t us = spec_hap.rfind('_');
        Cluster cl;
        if (us == std::string::npos || !parse_small_int(spec_hap.data() + us + 1, spec_hap.data() + spec_hap.size(), cl.number))
            return fail(MSNV_EFORMAT, "Species-cluster name did not conform to expectations. Expected something like: 537011_1 or ref_mOTU_v2_2227_1 where final number after "
                        "underscore is the cluster. Instead got: %s", spec_hap.c_str());
        if (int rc = profile_cluster(ctx, dir + name, dir + spec_hap + "_hap_positions.tab", samples, max_prop_uncalled, cl, ms_kernel)) return rc;
        if (cl.rows.size() >= 2) usable.push_back(std::move(cl));      // one kept column: "Insufficient data"; none: "No data"
    }
    if (result) result[2] = (int64_t)usable.size();
    if (usable.empty()) {
        if (result) result[0] = MSNV_PROFILE_NONE_USABLE;
        return append_line(stat_path, none_usable);
    }

    // ---- abundanceSummaryStats.tsv
    {
        std::string t = "Sample\tCluster\tmean\tmedian\tstandardDeviation\tprevalence\tprevalenceGte5\tn0\tn100\tnNoCoverage\n";
        for (const Cluster &cl : usable)
            for (const SummaryRow &r : cl.rows) {
                t += samples[r.sample]; t.push_back('\t'); t += std::to_string(cl.number); t.push_back('\t');
                r_double(r.mean, t); t.push_back('\t'); r_double(r.median, t); t.push_back('\t');
                if (r.sd_na) t += "NA"; else r_double(r.sd, t);
                t.push_back('\t'); r_double(r.prevalence, t); t.push_back('\t'); r_double(r.prevalence5, t); t.push_back('\t');
                t += std::to_string(r.n0); t.push_back('\t'); t += std::to_string(r.n100); t.push_back('\t'); t += std::to_string(r.n_na); t.push_back('\n');
            }
        if (int rc = write_text(prefix + "_abundanceSummaryStats.tsv", t)) return rc;
    }

    // ---- rmNAandSpread: the samples every usable cluster kept, in cluster 1's order (the sample order); a column of medians per cluster
    const size_t K = usable.size(), S = samples.size();
    std::vector<uint32_t> seen_in(S, 0);
    for (const Cluster &cl : usable) for (const SummaryRow &r : cl.rows) ++seen_in[r.sample];
    bool has_one = false;
    for (const Cluster &cl : usable) has_one = has_one || cl.number == 1;
    if (!has_one)
        return fail(MSNV_EDOMAIN, "species %s: cluster 1 is not among the usable clusters; the reference takes the table's samples from cluster 1 and binds columns of different "
                    "samples without it (the summary table is written)", species);
    std::vector<uint32_t> full;                                        // sample indices
    for (size_t s = 0; s < S; ++s) if (seen_in[s] == K) full.push_back((uint32_t)s);
    if (full.empty())
        return fail(MSNV_EDOMAIN, "species %s: no sample has a median in every usable cluster; the reference binds columns of different samples then (the summary table is "
                    "written)", species);
    std::vector<double> med(full.size() * K);
    std::vector<uint8_t> is_bad(S, 0);
    size_t n_bad = 0;
    for (size_t k = 0; k < K; ++k) {
        std::vector<int64_t> at(S, -1);
        for (size_t i = 0; i < usable[k].rows.size(); ++i) {
            const SummaryRow &r = usable[k].rows[i];
            at[r.sample] = (int64_t)i;
            if (r.median > 30.0 && r.prevalence < 0.75 && !is_bad[r.sample]) { is_bad[r.sample] = 1; ++n_bad; }
        }
        for (size_t i = 0; i < full.size(); ++i) med[i * K + k] = usable[k].rows[(size_t)at[full[i]]].median;
    }
    std::vector<uint32_t> coherent;                                    // indices into full
    size_t n_low = 0, n_multi = 0;
    for (size_t i = 0; i < full.size(); ++i) {
        long double s = 0;
        for (size_t k = 0; k < K; ++k) s += med[i * K + k];
        const double sum = (double)s;
        n_low += sum < 80.0; n_multi += sum > 120.0;
        if (sum >= 80.0 && sum <= 120.0) coherent.push_back((uint32_t)i);
    }
    if (n_low + n_multi > 0)
        if (int rc = append_line(stat_path, "Species " + sp + ": " + std::to_string(n_low + n_multi) + " out of " + std::to_string(full.size()) +
                                 " samples rejected due to incoherent subpecies assignment. Number of samples where summed abundance of clusters was < 80%: " +
                                 std::to_string(n_low) + ". Number of samples where summed abundance of clusters was > 120%:" + std::to_string(n_multi))) return rc;
    std::vector<uint32_t> filtered;
    if (n_bad > 0) {
        if (int rc = append_line(stat_path, "Species " + sp + ": " + std::to_string(n_bad) + " out of " + std::to_string(coherent.size()) +
                                 " samples rejected due to extreme mismatch between median abundance of genotyping SNVs (>30%) and prevalence of genotyping SNVs (<75%).")) return rc;
        for (uint32_t i : coherent) if (!is_bad[full[i]]) filtered.push_back(i);
    } else filtered = coherent;

    std::string header;
    for (size_t k = 0; k < K; ++k) { if (k) header.push_back('\t'); header += std::to_string(usable[k].number); }
    header.push_back('\n');
    auto table = [&](const std::vector<uint32_t> &rows_) {
        std::string t = header;
        for (uint32_t i : rows_) {
            t += samples[full[i]];
            for (size_t k = 0; k < K; ++k) { t.push_back('\t'); r_double(med[i * K + k], t); }
            t.push_back('\n');
        }
        return t;
    };
    std::vector<uint32_t> all_rows(full.size());
    for (size_t i = 0; i < full.size(); ++i) all_rows[i] = (uint32_t)i;
    if (int rc = write_text(prefix + "_wFreq_unfiltered.tab", table(all_rows))) return rc;
    if (int rc = write_text(prefix + "_wFreq.tab", table(filtered))) return rc;
    std::string t = "clust\n";
    uint64_t n_assigned = 0;
    for (uint32_t i : filtered) {
        size_t above = 0, which = 0;
        for (size_t k = 0; k < K; ++k) if (med[i * K + k] > min_genotype_abundance) { ++above; which = k + 1; }
        t += samples[full[i]]; t.push_back('\t');
        if (above == 1) { t += std::to_string(which); ++n_assigned; } else t += "NA";
        t.push_back('\n');
    }
    if (int rc = write_text(prefix + ".tab", t)) return rc;
    if (result) {
        result[0] = MSNV_PROFILE_OK; result[3] = (int64_t)full.size(); result[4] = (int64_t)filtered.size(); result[5] = (int64_t)(n_low + n_multi);
        result[6] = (int64_t)n_bad; result[7] = (int64_t)n_assigned;
    }
    return MSNV_OK;
}

extern "C" int msnv_subpop_abundance_files(const char *species, const char *out_dir, const char *abundance_path, const char *sample_suffix, uint64_t counts[4]) {
    clear_error();
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!species || !out_dir || !abundance_path) return fail(MSNV_EINVAL, "msnv_subpop_abundance_files: NULL argument");
    const std::string sp = species, dir = std::string(out_dir) + "/", freq_path = dir + sp + "_extended_clustering_wFreq.tab";

    // ---- wFreq.tab: write.table's layout, the header one field short; check.names puts an X before a number
    std::string text;
    if (int rc = slurp(freq_path, text)) return rc;
    std::vector<std::string> cnames, fsamples;
    std::vector<double> freq;                                          // [sample][K]
    uint64_t lineno = 0;
    for (const std::string &ln : lines_of(text)) {
        const std::vector<std::string> f = split(ln, '\t');
        if (++lineno == 1) { for (const std::string &n : f) cnames.push_back(r_make_name(n)); continue; }
        if (f.size() != cnames.size() + 1) return fail(MSNV_EFORMAT, "%s:%llu: %zu fields, the header names %zu clusters", freq_path.c_str(), (unsigned long long)lineno, f.size(), cnames.size());
        fsamples.push_back(f[0]);
        for (size_t k = 1; k < f.size(); ++k) {
            double v;
            if (!parse_number(f[k], v)) return fail(MSNV_EFORMAT, "%s:%llu: '%s' is not a number", freq_path.c_str(), (unsigned long long)lineno, f[k].c_str());
            freq.push_back(v);
        }
    }
    const size_t K = cnames.size();
    if (counts) { counts[1] = K; counts[2] = fsamples.size(); }

    // ---- the species abundance table: '#' comments, the first line the sample names, the first column the species
    text.clear();
    if (int rc = slurp(abundance_path, text)) return rc;
    std::vector<std::string> tnames, row;
    size_t n_match = 0;
    bool have_header = false;
    for (std::string ln : lines_of(text)) {
        const size_t hash = ln.find('#');
        if (hash != std::string::npos) ln.erase(hash);
        if (ln.find_first_not_of(" \t") == std::string::npos) continue;
        std::vector<std::string> f = split(ln, '\t');
        if (!have_header) { have_header = true; tnames.assign(f.begin() + 1, f.end()); continue; }
        if (f[0] == sp && ++n_match == 1) row = std::move(f);
    }
    if (counts) counts[3] = tnames.size();
    if (n_match == 0) return fail(MSNV_EDOMAIN, "Species not found in the species abundance profile. Species: %s", species);
    if (n_match > 1) return fail(MSNV_EDOMAIN, "More than one species in the abundance profile matched for species named: %s", species);
    if (fsamples.empty()) return fail(MSNV_EDOMAIN, "Species does not have cluster frequencies. Species: %s", species);
    if (row.size() != tnames.size() + 1) return fail(MSNV_EFORMAT, "%s: the row of %s has %zu cells, the first line names %zu samples", abundance_path, species, row.size() - 1, tnames.size());

    // ---- the samples both hold, in the table's column order; with none and a suffix given, the table's names with the suffix appended
    std::unordered_map<std::string, size_t> frow;
    for (size_t i = 0; i < fsamples.size(); ++i) frow.emplace(fsamples[i], i);
    std::vector<std::pair<size_t, size_t>> use;                        // (table column, wFreq row)
    for (int attempt = 0; attempt < 2 && use.empty(); ++attempt) {
        if (attempt == 1 && !sample_suffix) break;
        std::unordered_set<std::string> taken;
        for (size_t c = 0; c < tnames.size(); ++c) {
            const std::string name = attempt ? tnames[c] + sample_suffix : tnames[c];
            auto it = frow.find(name);
            if (it != frow.end() && taken.insert(name).second) use.emplace_back(c, it->second);
        }
    }
    if (use.empty())
        return fail(MSNV_EDOMAIN, "No overlapping sample IDs between clustering and apecies abundance profiles. Are IDs formatted differently? Example clustering IDs: %s. "
                    "Example species profile IDs:%s", last_three(fsamples).c_str(), last_three(tnames).c_str());
    std::vector<double> abund(use.size());
    for (size_t i = 0; i < use.size(); ++i)
        if (!parse_number(row[use[i].first + 1], abund[i]))
            return fail(MSNV_EFORMAT, "%s: the abundance of %s in sample %s, '%s', is not a number", abundance_path, species, tnames[use[i].first].c_str(), row[use[i].first + 1].c_str());

    // ---- clusterFreqs / 100 * speciesProfile, in that order
    auto table = [&](size_t k0, size_t k1) {
        std::string t;
        for (size_t k = k0; k < k1; ++k) { if (k > k0) t.push_back('\t'); t += cnames[k]; }
        t.push_back('\n');
        for (size_t i = 0; i < use.size(); ++i) {
            t += fsamples[use[i].second];
            for (size_t k = k0; k < k1; ++k) { t.push_back('\t'); r_double(freq[use[i].second * K + k] / 100.0 * abund[i], t); }
            t.push_back('\n');
        }
        return t;
    };
    if (int rc = write_text(dir + sp + "_allClust_relativeAbund.tab", table(0, K))) return rc;
    for (size_t k = 0; k < K; ++k)
        if (int rc = write_text(dir + sp + "_clust_" + std::to_string(k + 1) + "_hap_coverage_extended_normed.tab", table(k, k + 1))) return rc;
    if (counts) counts[0] = use.size();
    return MSNV_OK;
}
