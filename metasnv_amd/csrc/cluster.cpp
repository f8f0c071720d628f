// metasnv_amd/csrc/cluster.cpp -- host side of subpopr's computeClusters -> getClusteringResult (src/subpopr/R/clustering.R:20-133, :289-427;
// the kernels are cluster_k.hip).
//
//   msnv_pam_tasks       cluster::pam of many index subsets of one distance matrix
//   msnv_pred_strength   predStrengthCustom (:152-216) for given permutations, with mean.pred and optimalk
//   msnv_cluster_file(_ex)  the stage: outliers (filterSamples.R:42-72), SNV frequency composition (computeSnvFreqStats.R:1-24, :139-147), Gmax
//                        (:218-236), prediction strength, PAM, the stability of the cluster number (:359-381, clusteringStability.R:6-24,
//                        :201-221), small clusters (:383-400), the files
//   msnv_cluster_boot    fpc::clusterboot(bootmethod = "subset") on given subsets: PAM of the members and of every subset, each original cluster's
//                        best Jaccard match per subset as integers
//   msnv_membership_stability_file   the stability of each cluster's membership (clusteringStability.R:129-148, :170-176, :224-237) on the
//                        matrix msnv_cluster_file wrote: the two stability files (at the end of this file)
// What is on the host: reading and writing, the outlier rule (n numbers), the draws (include/msnv.h), R's mean() of each k's M values and the
// stability score.  Every PAM run, classification and pair count is on the device; there is no CPU fallback.
// Divergences: an NA cell is MSNV_EFORMAT here (rmNAfromDistMatrix is the driver's, metasnv_amd/subpopr_run.py); R's generator
// is not reproduced; when Gmax <= 1 no _PS_values.tab is written (the reference hands write.table a NULL there); a stability group that holds an NA
// does not count as constant.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "dataset.h"
#include "device.h"

namespace msnv {

// ---- what msnv_pcoa and msnv_pcoa_file (pcoa.cpp) share with this file (device.h)
int check_matrix(const char *who, int64_t n, const double *d) {
    if (n < 2 || n > (int64_t)CLUSTER_MAX_SAMPLES) return fail(MSNV_EDOMAIN, "%s: %lld samples (2 to %u)", who, (long long)n, CLUSTER_MAX_SAMPLES);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            const double v = d[i * n + j];
            if (!(v >= 0.0) || !std::isfinite(v)) return fail(MSNV_EDOMAIN, "%s: the distance of samples %lld and %lld is %g (distances are finite and >= 0)", who, (long long)i, (long long)j, v);
            if (v != d[j * n + i]) return fail(MSNV_EDOMAIN, "%s: the matrix is not symmetric at (%lld, %lld)", who, (long long)i, (long long)j);
            if (i == j && v != 0.0) return fail(MSNV_EDOMAIN, "%s: the diagonal is %g at sample %lld, not 0", who, v, (long long)i);
        }
    return MSNV_OK;
}

// <species>.filtered.mann.dist as write_matrix of dist.cpp writes it: a header of names behind an empty cell, then name + n cells per row.
// r_form: the header as write.table prints it (write_dist below), n names and no leading cell.
int read_dist(const char *path, std::vector<std::string> &names, std::vector<double> &d, bool r_form) {
    FILE *in = fopen(path, "r");
    if (!in) return fail(MSNV_EIO, "Cannot open %s: %s", path, strerror(errno));
    char *line = nullptr; size_t cap = 0; ssize_t len;
    uint64_t lineno = 0, n_rows = 0;
    int rc = MSNV_OK;
    while (rc == MSNV_OK && (len = getline(&line, &cap, in)) >= 0) {
        ++lineno;
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (lineno > 1 && len == 0) continue;
        std::vector<std::string> f;
        const char *s = line, *end = line + len;
        while (true) {
            const char *t = (const char *)memchr(s, '\t', (size_t)(end - s));
            f.emplace_back(s, t ? t : end);
            if (!t) break;
            s = t + 1;
        }
        if (lineno == 1) { names.assign(f.begin() + (r_form ? 0 : 1), f.end()); continue; }
        if (f.size() != names.size() + 1) { rc = fail(MSNV_EFORMAT, "%s:%llu: %zu cells for %zu samples", path, (unsigned long long)lineno, f.size() - 1, names.size()); break; }
        if (n_rows >= names.size() || f[0] != names[n_rows]) { rc = fail(MSNV_EFORMAT, "%s:%llu: row '%s' does not follow the header's order", path, (unsigned long long)lineno, f[0].c_str()); break; }
        for (size_t c = 1; c < f.size(); ++c) {
            char *e = nullptr;
            const double v = f[c].empty() || f[c] == "NA" ? 0.0 : strtod(f[c].c_str(), &e);
            if (!e || e != f[c].c_str() + f[c].size()) { rc = fail(MSNV_EFORMAT, "%s:%llu: cell '%s' is not a number (NA and empty cells are refused: metaSNV_subpopr.py removes them before the stages, rmNAfromDistMatrix)", path, (unsigned long long)lineno, f[c].c_str()); break; }
            d.push_back(v);
        }
        ++n_rows;
    }
    free(line);
    fclose(in);
    if (rc) return rc;
    if (n_rows != names.size()) return fail(MSNV_EFORMAT, "%s: %llu rows for %zu samples", path, (unsigned long long)n_rows, names.size());
    return MSNV_OK;
}

// removeOutliersFromDistMatrixMinDissim(maxTimesSd = 3, maxNoutliers = 5) (filterSamples.R:42-72): the samples that stay, in matrix order.  A sample
// whose smallest distance to another lies more than 3 sd from the mean of those is an outlier; none or more than 5 of them: everybody stays.
std::vector<int32_t> remove_outliers(const std::vector<double> &d, size_t n_all) {
    std::vector<double> mind(n_all);
    for (size_t i = 0; i < n_all; ++i) {
        double m = INFINITY;
        for (size_t j = 0; j < n_all; ++j) if (j != i) m = std::min(m, d[i * n_all + j]);
        mind[i] = m;
    }
    const double mean = r_mean(mind.data(), n_all), sd = r_sd(mind.data(), n_all), hi = mean + 3 * sd, lo = mean - 3 * sd;
    std::vector<int32_t> keep, all(n_all);
    for (size_t i = 0; i < n_all; ++i) { all[i] = (int32_t)i; if (!(mind[i] > hi || mind[i] < lo)) keep.push_back((int32_t)i); }
    const size_t n_out = n_all - keep.size();
    return (n_out == 0 || n_out > 5) ? all : keep;
}

namespace {

// ---- the draws (include/msnv.h)
inline uint64_t mix(uint64_t x) {
    uint64_t z = x + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
inline uint64_t draw(uint64_t seed, uint64_t ordinal, uint64_t i) { return mix(mix(mix(seed) + ordinal) + i); }
void permutation(uint64_t seed, uint64_t ordinal, uint32_t n, std::vector<int32_t> &p) {
    p.resize(n);
    for (uint32_t i = 0; i < n; ++i) p[i] = (int32_t)i;
    for (uint32_t i = n; i-- > 1;) std::swap(p[i], p[draw(seed, ordinal, i) % (i + 1)]);
}

// mean.pred and optimalk from the prederr of one run (k = 2..gmax, M values each)
void ps_summary(const double *prederr, uint32_t gmax, uint32_t M, double cutoff, std::vector<double> &mean_pred, int32_t &optimalk) {
    mean_pred.assign(gmax, 1.0);
    optimalk = 0;
    for (uint32_t k = 2; k <= gmax; ++k) mean_pred[k - 1] = r_mean(prederr + (size_t)(k - 2) * M, M);
    for (uint32_t k = 1; k <= gmax; ++k) if (mean_pred[k - 1] > cutoff) optimalk = (int32_t)k;
}

// The subsample proportions of both stability assessments (clustering.R:359-381): from the proportion that leaves 10 samples, 0.3 at the least, to
// 1 in steps of 0.1, each with its subsample size.  n >= 10.
struct SubsampleStep { double prop; uint32_t size; };
std::vector<SubsampleStep> subsample_steps(uint32_t n) {
    std::vector<SubsampleStep> steps;
    const double low = std::max(0.3, std::ceil(10.0 / n * 10) / 10);
    for (uint32_t pi = 0;; ++pi) {
        const double prop = low + pi * 0.1;
        if (!(prop <= 1 + 1e-10)) break;
        steps.push_back(SubsampleStep{prop, std::min(n, (uint32_t)std::floor(n * prop))});
    }
    return steps;
}

uint32_t max_clusters_to_try(uint32_t n, uint32_t dflt, uint32_t min_size) {      // getMaxNumClustersToTry (:218-236); may be "negative": 0
    const int64_t a = (int64_t)(n / 2) - 1, b = n / min_size, lim = std::min(a, b);
    return (uint32_t)std::max<int64_t>(0, std::min<int64_t>(dflt, lim));
}

// the splits of several prediction-strength runs, gathered for one launch
struct Splits {
    std::vector<uint32_t> len, k;
    std::vector<int32_t> idx;
    // every (k, l) of one run over `members` (global indices): the permutation's ordinal is ord_base + (k - 2) * M + l
    void add_run(const std::vector<int32_t> &members, uint32_t gmax, uint32_t M, uint64_t seed, uint64_t ord_base) {
        std::vector<int32_t> p;
        for (uint32_t kk = 2; kk <= gmax; ++kk)
            for (uint32_t l = 0; l < M; ++l) {
                permutation(seed, ord_base + (uint64_t)(kk - 2) * M + l, (uint32_t)members.size(), p);
                len.push_back((uint32_t)members.size()); k.push_back(kk);
                for (int32_t q : p) idx.push_back(members[q]);
            }
    }
};

// write.table(as.matrix(d), sep = "\t", quote = F) of the samples `members` of the matrix
int write_dist(const std::string &path, const std::vector<std::string> &names, const std::vector<double> &d, size_t n, const std::vector<int32_t> &members) {
    std::string text;
    for (size_t a = 0; a < members.size(); ++a) { if (a) text.push_back('\t'); text += names[members[a]]; }
    text.push_back('\n');
    for (int32_t i : members) {
        text += names[i];
        for (int32_t j : members) { text.push_back('\t'); r_double(d[(size_t)i * n + j], text); }
        text.push_back('\n');
    }
    return write_text(path, text);
}

// getNClusStabScore (clusteringStability.R:201-221).  num < 0 = NA; a group that is empty, single or holds an NA is not "constant"
int stab_score(const std::vector<double> &prop, const std::vector<int32_t> &num) {
    auto group = [&](long tenth, bool &constant, int32_t &first) {
        size_t cnt = 0;
        constant = true; first = -1;
        for (size_t i = 0; i < prop.size(); ++i)
            if (std::lround(prop[i] * 10.0) == tenth) {
                if (cnt == 0) first = num[i];
                if (num[i] < 0 || num[i] != first) constant = false;
                ++cnt;
            }
        if (cnt < 2) constant = false;
    };
    bool c100, c90, c80; int32_t n100, n90, n80;
    group(10, c100, n100);
    if (!c100) return 1;
    group(9, c90, n90); group(8, c80, n80);
    return (c90 && c80 && n90 == n100 && n80 == n100) ? 3 : 2;
}

}  // namespace
}  // namespace msnv

using namespace msnv;

extern "C" void msnv_cluster_opts_default(msnv_cluster_opts *o) { if (o) *o = msnv_cluster_opts{1, 0.8, 10, 0}; }

extern "C" int msnv_pam_tasks(msnv_ctx *ctx, int32_t n, const double *dist, int64_t n_tasks, const int32_t *task_m, const int32_t *task_k, const int32_t *idx,
                              int32_t *medoids, int32_t *cluster, int32_t *n_swaps, double *ms_kernel) {
    clear_error();
    if (!ctx || !dist || n_tasks < 0 || (n_tasks && (!task_m || !task_k || !idx || !medoids || !cluster || !n_swaps))) return fail(MSNV_EINVAL, "msnv_pam_tasks: NULL argument or a negative count");
    if (ms_kernel) *ms_kernel = 0;
    if (int rc = check_matrix("msnv_pam_tasks", n, dist)) return rc;
    std::vector<uint32_t> m((size_t)n_tasks), k((size_t)n_tasks);
    uint64_t off = 0;
    for (int64_t t = 0; t < n_tasks; ++t) {
        if (task_m[t] < 2 || task_m[t] > n || task_k[t] < 1 || task_k[t] >= task_m[t])
            return fail(MSNV_EDOMAIN, "msnv_pam_tasks: task %lld has m = %d, k = %d (2 <= m <= n, 1 <= k < m)", (long long)t, task_m[t], task_k[t]);
        for (int32_t j = 0; j < task_m[t]; ++j)
            if (idx[off + j] < 0 || idx[off + j] >= n) return fail(MSNV_EDOMAIN, "msnv_pam_tasks: task %lld lists sample %d of %d", (long long)t, idx[off + j], n);
        m[t] = (uint32_t)task_m[t]; k[t] = (uint32_t)task_k[t]; off += m[t];
    }
    if (int rc = dev_set_device(ctx->device)) return rc;
    if (n_tasks == 0) return MSNV_OK;
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, dist, (uint32_t)n, ctx->stream)) return rc;
    return dev_pam_tasks(dev, (uint64_t)n_tasks, m.data(), k.data(), idx, ctx->stream, medoids, cluster, n_swaps, ms_kernel);
}

extern "C" int msnv_pred_strength(msnv_ctx *ctx, int32_t n, const double *dist, int32_t k_max, int32_t M, const int32_t *perms, double cutoff, double *prederr,
                                  double *mean_pred, int32_t *optimalk, double *ms_kernel) {
    clear_error();
    if (!ctx || !dist || !perms || !prederr || !mean_pred || !optimalk) return fail(MSNV_EINVAL, "msnv_pred_strength: NULL argument");
    if (ms_kernel) *ms_kernel = 0;
    if (M < 1 || !(cutoff >= 0.0 && cutoff < 1.0)) return fail(MSNV_EINVAL, "msnv_pred_strength: M = %d, cutoff = %g (M >= 1, 0 <= cutoff < 1)", M, cutoff);
    if (int rc = check_matrix("msnv_pred_strength", n, dist)) return rc;
    if (k_max < 2 || k_max >= n / 2) return fail(MSNV_EDOMAIN, "msnv_pred_strength: k_max = %d with halves of %d samples (2 <= k_max < floor(n / 2))", k_max, n / 2);
    const size_t n_splits = (size_t)(k_max - 1) * M;
    std::vector<uint8_t> seen((size_t)n);
    std::vector<uint32_t> len(n_splits, (uint32_t)n), k(n_splits);
    for (size_t s = 0; s < n_splits; ++s) {
        k[s] = (uint32_t)(2 + s / M);
        std::fill(seen.begin(), seen.end(), 0);
        for (int32_t j = 0; j < n; ++j) {
            const int32_t v = perms[s * n + j];
            if (v < 0 || v >= n || seen[v]) return fail(MSNV_EDOMAIN, "msnv_pred_strength: permutation %zu is not a permutation of 0..%d", s, n - 1);
            seen[v] = 1;
        }
    }
    if (int rc = dev_set_device(ctx->device)) return rc;
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, dist, (uint32_t)n, ctx->stream)) return rc;
    if (int rc = dev_pred_strength(dev, n_splits, len.data(), k.data(), perms, ctx->stream, prederr, ms_kernel)) return rc;
    std::vector<double> mp;
    ps_summary(prederr, (uint32_t)k_max, (uint32_t)M, cutoff, mp, *optimalk);
    memcpy(mean_pred, mp.data(), mp.size() * 8);
    return MSNV_OK;
}

extern "C" void msnv_cluster_filter_default(msnv_cluster_filter *f) { if (f) *f = msnv_cluster_filter{0.1, 0.8}; }

extern "C" int msnv_cluster_file(msnv_ctx *ctx, const char *dist_path, const char *freq_path, const char *species, const char *out_dir, const msnv_cluster_opts *opts,
                                 int64_t result[8], double *ms_kernel) {
    return msnv_cluster_file_ex(ctx, dist_path, freq_path, species, out_dir, opts, nullptr, result, ms_kernel);
}

extern "C" int msnv_cluster_file_ex(msnv_ctx *ctx, const char *dist_path, const char *freq_path, const char *species, const char *out_dir, const msnv_cluster_opts *opts,
                                    const msnv_cluster_filter *filter, int64_t result[8], double *ms_kernel) {
    clear_error();
    if (!ctx || !dist_path || !species || !out_dir) return fail(MSNV_EINVAL, "msnv_cluster_file: NULL argument");
    msnv_cluster_opts o;
    msnv_cluster_opts_default(&o);
    if (opts) o = *opts;
    if (o.reserved != 0 || o.stability_iters < 1 || o.stability_iters > 1024 || !(o.ps_cut >= 0.0 && o.ps_cut < 1.0))
        return fail(MSNV_EINVAL, "msnv_cluster_file: ps_cut = %g, stability_iters = %d, reserved = %d (0 <= ps_cut < 1, 1..1024 iterations, reserved 0)", o.ps_cut, o.stability_iters, o.reserved);
    msnv_cluster_filter flt;
    msnv_cluster_filter_default(&flt);
    if (filter) flt = *filter;
    if (!(flt.max_prop_reads_non_homog >= 0.0 && flt.max_prop_reads_non_homog <= 1.0) || !(flt.min_prop_homog_snv >= 0.0 && flt.min_prop_homog_snv <= 1.0))
        return fail(MSNV_EINVAL, "msnv_cluster_file_ex: max_prop_reads_non_homog = %g, min_prop_homog_snv = %g (0 <= proportion <= 1)", flt.max_prop_reads_non_homog,
                    flt.min_prop_homog_snv);
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    double ms = 0;
    const uint32_t M = 50;
    std::vector<std::string> names;
    std::vector<double> d;
    if (int rc = read_dist(dist_path, names, d)) return rc;
    const size_t n_all = names.size();
    if (int rc = check_matrix(dist_path, (int64_t)n_all, d.data())) return rc;
    if (int rc = dev_set_device(ctx->device)) return rc;
    const std::string out = std::string(out_dir) + "/", failed_dir = out + "clustMedoidDefnFailed/", none_dir = out + "noClustering/";
    const std::string prefix = std::string(species) + "_mann";
    if (int rc = make_dir(out_dir)) return rc;

    // ---- removeOutliersFromDistMatrixMinDissim(maxTimesSd = 3, maxNoutliers = 5)
    const std::vector<int32_t> qc = remove_outliers(d, n_all);         // samples after outlier removal, in matrix order
    if (result) result[3] = (int64_t)(n_all - qc.size());
    if (qc.size() < 2) return fail(MSNV_EDOMAIN, "%s: %zu samples left after outlier removal", dist_path, qc.size());

    // ---- computeSnvFreqStats, computeSnvFreqStatsThreshold(-x) + onlyKeepSamplesWithDistinctFreqs(-y) (clustering.R:41-79)
    std::vector<int32_t> used = qc;                                    // distForMedoids
    std::string composition;
    if (freq_path) {
        std::vector<std::string> fnames;
        std::vector<double> rows;
        uint64_t n_pos = 0;
        if (int rc = read_freq(freq_path, fnames, nullptr, rows, n_pos)) return rc;
        const size_t S = fnames.size();
        if (S == 0) return fail(MSNV_EFORMAT, "%s: no sample column", freq_path);
        if (S > 0x7fffffffull) return fail(MSNV_EDOMAIN, "%s: %zu sample columns", freq_path, S);
        std::vector<uint64_t> cnt(S * 4, 0);
        if (int rc = dev_freq_bands(rows.data(), n_pos, (uint32_t)S, ctx->stream, cnt.data(), &ms)) return rc;
        composition = "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95\n";
        for (size_t s = 0; s < S; ++s) {
            const double valid = (double)cnt[s * 4 + 3];
            composition += fnames[s];
            for (int b = 0; b < 3; ++b) { composition.push_back('\t'); r_double((double)cnt[s * 4 + b] / valid, composition); }
            composition.push_back('\n');
        }
        // computeSnvFreqStatsThreshold's band of -x: the strict count of msnv_freq_curves_k ([101] of a sample's 102, covered cells in [100])
        const bool filtering = flt.min_prop_homog_snv > 0.0;           // clustering.R:47: doFilterSamplesByAlleleDist & minPropHomogSnvAllelesPerSample > 0
        if (filtering) {
            double lo = 0, hi = 0;
            strict_band(flt.max_prop_reads_non_homog, lo, hi);
            std::vector<uint64_t> curves(S * 102, 0);
            if (n_pos) {
                uint32_t outside = 0;
                if (int rc = dev_freq_curves(rows.data(), n_pos, (uint32_t)S, lo, hi, ctx->stream, curves.data(), &outside, &ms)) return rc;
                if (outside) return fail(MSNV_EDOMAIN, "%s: a cell is neither -1 nor within [0, 100]", freq_path);
            }
            std::unordered_map<std::string, int32_t> in_qc;
            for (int32_t i : qc) in_qc.emplace(names[i], i);
            used.clear();
            for (size_t s = 0; s < S; ++s) {
                auto it = in_qc.find(fnames[s]);
                if ((double)curves[s * 102 + 101] / (double)curves[s * 102 + 100] >= flt.min_prop_homog_snv && it != in_qc.end()) { used.push_back(it->second); in_qc.erase(it); }
            }
        }
        int status = -1;
        if (filtering && used.size() < 6) status = MSNV_CLUSTER_TOO_FEW;
        else if (filtering) {
            bool all_equal = true;
            const double v0 = d[(size_t)used[1] * n_all + used[0]];
            for (size_t a = 1; a < used.size() && all_equal; ++a)
                for (size_t b = 0; b < a; ++b) if (d[(size_t)used[a] * n_all + used[b]] != v0) { all_equal = false; break; }
            if (all_equal) status = MSNV_CLUSTER_ALL_EQUAL;
        }
        if (status >= 0) {
            if (int rc = make_dir(failed_dir)) return rc;
            if (int rc = write_text(failed_dir + species + "_freq_composition.tab", composition)) return rc;
            if (result) { result[0] = status; result[2] = (int64_t)used.size(); }
            if (ms_kernel) *ms_kernel = ms;
            return MSNV_OK;
        }
    }
    const uint32_t n = (uint32_t)used.size();

    // ---- getClusPredStrengthResult(defaultMaxNumClusters = 15, minClusterSize = 3), then pam on everything
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, d.data(), (uint32_t)n_all, ctx->stream)) return rc;
    const uint32_t gmax = max_clusters_to_try(n, 15, 3);
    std::vector<double> mean_pred;
    int32_t optimalk = 1;
    uint64_t n_tasks = 1;
    if (gmax > 1) {
        Splits sp;
        sp.add_run(used, gmax, M, o.seed, 0);
        std::vector<double> prederr(sp.len.size());
        if (int rc = dev_pred_strength(dev, sp.len.size(), sp.len.data(), sp.k.data(), sp.idx.data(), ctx->stream, prederr.data(), &ms)) return rc;
        ps_summary(prederr.data(), gmax, M, o.ps_cut, mean_pred, optimalk);
        n_tasks += 2 * sp.len.size();
    }
    std::vector<int32_t> medoids((size_t)optimalk), clus(n);
    {
        const uint32_t m1 = n, k1 = (uint32_t)optimalk;
        int32_t swaps = 0;
        if (int rc = dev_pam_tasks(dev, 1, &m1, &k1, used.data(), ctx->stream, medoids.data(), clus.data(), &swaps, &ms)) return rc;
    }

    // ---- getClusNumStability: every subsample's prediction-strength run in one batch
    std::vector<double> stab_prop;
    std::vector<int32_t> stab_num;
    int score = 0;
    if (n >= 10) {
        const std::vector<SubsampleStep> steps = subsample_steps(n);
        Splits sp;
        struct Run { size_t first; uint32_t gmax; };
        std::vector<Run> runs;
        std::vector<int32_t> p, sub;
        for (uint32_t pi = 0; pi < steps.size(); ++pi) {
            const double prop = steps[pi].prop;
            const uint32_t size = steps[pi].size;
            for (int32_t it = 0; it < o.stability_iters; ++it) {
                const uint64_t r = 1 + 1024ull * pi + (uint64_t)it;
                permutation(o.seed, r << 32 | 0xffffffffull, n, p);
                sub.resize(size);
                for (uint32_t a = 0; a < size; ++a) sub[a] = used[p[a]];
                const uint32_t g = max_clusters_to_try(size, 10, 5);
                runs.push_back(Run{sp.len.size(), g});
                stab_prop.push_back(prop);
                if (g > 1) sp.add_run(sub, g, M, o.seed, r << 32);
            }
        }
        std::vector<double> prederr(sp.len.size());
        if (!sp.len.empty())
            if (int rc = dev_pred_strength(dev, sp.len.size(), sp.len.data(), sp.k.data(), sp.idx.data(), ctx->stream, prederr.data(), &ms)) return rc;
        n_tasks += 2 * sp.len.size();
        std::vector<double> mp;
        for (const Run &r : runs) {
            int32_t ok = -1;                                           // NA
            if (r.gmax > 1) ps_summary(prederr.data() + r.first, r.gmax, M, o.ps_cut, mp, ok);
            stab_num.push_back(ok);
        }
        score = stab_score(stab_prop, stab_num);
    }

    // ---- clusters under 3 members are dropped (:383-400)
    std::vector<uint32_t> sizes((size_t)optimalk + 1, 0);
    for (int32_t c : clus) ++sizes[c];
    uint32_t n_big = 0;
    for (int32_t c = 1; c <= optimalk; ++c) n_big += sizes[c] >= 3;
    const bool one = n_big <= 1;
    const std::string dir = one ? none_dir : out;
    if (one) if (int rc = make_dir(none_dir)) return rc;
    if (gmax <= 1) {
        if (int rc = make_dir(failed_dir)) return rc;
        if (int rc = write_dist(failed_dir + prefix + "_distMatrixUsedForClustMedoidDefns.txt", names, d, n_all, used)) return rc;
    } else {
        std::string text = "x\n";
        for (uint32_t k = 1; k <= gmax; ++k) { text += std::to_string(k); text.push_back('\t'); r_double(mean_pred[k - 1], text); text.push_back('\n'); }
        if (int rc = write_text(dir + prefix + "_PS_values.tab", text)) return rc;
    }
    if (int rc = write_dist(dir + prefix + "_distMatrixUsedForClustMedoidDefns.txt", names, d, n_all, used)) return rc;
    if (freq_path) if (int rc = write_text(dir + species + "_freq_composition.tab", composition)) return rc;
    {
        std::string text = "clust\n";
        if (one) for (int32_t i : qc) { text += names[i]; text += "\t1\n"; }           // getClustDf: every sample of the matrix after outlier removal
        else for (uint32_t a = 0; a < n; ++a) if (sizes[clus[a]] >= 3) { text += names[used[a]]; text.push_back('\t'); text += std::to_string(clus[a]); text.push_back('\n'); }
        if (int rc = write_text(dir + prefix + "_clustering.tab", text)) return rc;
    }
    if (!stab_prop.empty()) {
        std::string text = "propSamples\tnumClusters\n";
        for (size_t i = 0; i < stab_prop.size(); ++i) {
            r_double(stab_prop[i], text); text.push_back('\t');
            text += stab_num[i] < 0 ? std::string("NA") : std::to_string(stab_num[i]);
            text.push_back('\n');
        }
        if (int rc = write_text(dir + prefix + "_clusNumStability.tab", text)) return rc;
    }
    if (result) {
        result[0] = gmax <= 1 ? MSNV_CLUSTER_MEDOID_FAILED : one ? MSNV_CLUSTER_NONE : MSNV_CLUSTER_OK;
        result[1] = one ? 1 : n_big; result[2] = n; result[4] = score; result[5] = optimalk; result[6] = (int64_t)n_tasks;
    }
    if (ms_kernel) *ms_kernel = ms;
    return MSNV_OK;
}

// ---------------------------------------------------------------------------------------------- the stability of each cluster's membership
// getClusMembStability -> clusterAssignSubsample -> getClusMembStabScore (clusteringStability.R:129-148, :170-176, :224-237).  On the host: the
// draws, the quotients inter / union of the integers the device returns, R's mean() of them, the two counts, the score and the files.
namespace msnv {
namespace {

// the members clustered, then every subset re-clustered and matched: the input is valid.  best: [n_sets][k][2]
int boot_run(msnv_ctx *ctx, const ClusterDev &dev, const std::vector<int32_t> &members, uint32_t k, const std::vector<uint32_t> &set_m, const std::vector<int32_t> &set_pos,
             int32_t *medoids, int32_t *cluster, std::vector<int32_t> &best, double *ms) {
    std::vector<uint32_t> m{(uint32_t)members.size()};
    m.insert(m.end(), set_m.begin(), set_m.end());
    std::vector<int32_t> idx(members);
    idx.reserve(members.size() + set_pos.size());
    for (int32_t p : set_pos) idx.push_back(members[p]);
    best.assign(set_m.size() * k * 2, 0);
    return dev_cluster_boot(dev, set_m.size(), m.data(), k, idx.data(), set_pos.data(), ctx->stream, medoids, cluster, best.data(), ms);
}

struct MembRow { bool na; double jaccard, recover; };                  // one (proportion, cluster) of _clusMembStability.tab

// R's three-valued logic: 0 FALSE, 1 TRUE, 2 NA
int above3(const MembRow *r, double v, double thr) { return (!r || r->na || v != v) ? 2 : v > thr ? 1 : 0; }
int and3(int a, int b) { return (a == 0 || b == 0) ? 0 : (a == 2 || b == 2) ? 2 : 1; }

// getClusMembStabScore of cluster j (0-based): 1 Low, 2 Medium, 3 High, 0 NA
int memb_score(const std::vector<SubsampleStep> &steps, const std::vector<MembRow> &rows, uint32_t k, uint32_t j) {
    auto term = [&](long tenth, double thr) {
        const MembRow *r = nullptr;
        for (size_t pi = 0; pi < steps.size() && !r; ++pi) if (std::lround(steps[pi].prop * 10.0) == tenth) r = &rows[pi * k + j];
        return and3(above3(r, r ? r->recover : 0.0, thr), above3(r, r ? r->jaccard : 0.0, thr));
    };
    const int at90 = term(9, 0.8), at70 = term(7, 0.9);
    return (at90 == 2 || at70 == 2) ? 0 : 1 + at90 + at70;
}

// <species>_mann_clusNumStability.tab as msnv_cluster_file writes it; num < 0 = NA
int read_num_stability(const char *path, std::vector<double> &prop, std::vector<int32_t> &num) {
    FILE *in = fopen(path, "r");
    if (!in) return fail(MSNV_EIO, "Cannot open %s: %s", path, strerror(errno));
    char *line = nullptr; size_t cap = 0; ssize_t len;
    uint64_t lineno = 0;
    int rc = MSNV_OK;
    while (rc == MSNV_OK && (len = getline(&line, &cap, in)) >= 0) {
        ++lineno;
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (lineno == 1 || len == 0) continue;
        char *e = nullptr;
        const double p = strtod(line, &e);
        if (e == line || *e != '\t') { rc = fail(MSNV_EFORMAT, "%s:%llu: a proportion and a cluster number are expected", path, (unsigned long long)lineno); break; }
        const char *cell = e + 1;
        long v = -1;
        if (strcmp(cell, "NA") != 0) {
            v = strtol(cell, &e, 10);
            if (e == cell || *e || v < 0 || v > INT32_MAX) { rc = fail(MSNV_EFORMAT, "%s:%llu: cluster number '%s'", path, (unsigned long long)lineno, cell); break; }
        }
        prop.push_back(p); num.push_back((int32_t)v);
    }
    free(line);
    fclose(in);
    return rc;
}

const char *const SCORE_NAMES[4] = {"NA", "Low", "Medium", "High"};

}  // namespace
}  // namespace msnv

extern "C" void msnv_membstab_opts_default(msnv_membstab_opts *o) { if (o) *o = msnv_membstab_opts{1, 100, 0}; }

extern "C" int msnv_cluster_boot(msnv_ctx *ctx, int32_t n, const double *dist, int32_t m, const int32_t *members, int32_t k, int64_t n_sets, const int32_t *set_m,
                                 const int32_t *set_pos, int32_t *medoids, int32_t *cluster, int32_t *best_inter, int32_t *best_union, double *ms_kernel) {
    clear_error();
    if (!ctx || !dist || !members || !medoids || !cluster || n_sets < 0 || (n_sets && (!set_m || !set_pos || !best_inter || !best_union)))
        return fail(MSNV_EINVAL, "msnv_cluster_boot: NULL argument or a negative count");
    if (ms_kernel) *ms_kernel = 0;
    if (int rc = check_matrix("msnv_cluster_boot", n, dist)) return rc;
    if (m < 2 || m > n) return fail(MSNV_EDOMAIN, "msnv_cluster_boot: %d members of %d samples (2 <= m <= n)", m, n);
    for (int32_t a = 0; a < m; ++a)
        if (members[a] < 0 || members[a] >= n || (a && members[a] <= members[a - 1]))
            return fail(MSNV_EDOMAIN, "msnv_cluster_boot: member %d is sample %d (0 <= sample < %d, ascending)", a, members[a], n);
    if (k < 1 || k > (int32_t)CLUSTER_BOOT_MAX_K || k >= m) return fail(MSNV_EDOMAIN, "msnv_cluster_boot: k = %d with %d members (1 <= k <= %u, k < m)", k, m, CLUSTER_BOOT_MAX_K);
    std::vector<int64_t> seen((size_t)m, -1);
    std::vector<uint32_t> sm((size_t)n_sets);
    uint64_t off = 0;
    for (int64_t t = 0; t < n_sets; ++t) {
        if (set_m[t] <= k || set_m[t] > m) return fail(MSNV_EDOMAIN, "msnv_cluster_boot: subset %lld has %d entries (k = %d < entries <= m = %d)", (long long)t, set_m[t], k, m);
        for (int32_t e = 0; e < set_m[t]; ++e) {
            const int32_t p = set_pos[off + e];
            if (p < 0 || p >= m) return fail(MSNV_EDOMAIN, "msnv_cluster_boot: subset %lld lists position %d of %d", (long long)t, p, m);
            if (seen[p] == t) return fail(MSNV_EDOMAIN, "msnv_cluster_boot: subset %lld lists position %d twice", (long long)t, p);
            seen[p] = t;
        }
        sm[t] = (uint32_t)set_m[t]; off += sm[t];
    }
    if (int rc = dev_set_device(ctx->device)) return rc;
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, dist, (uint32_t)n, ctx->stream)) return rc;
    std::vector<int32_t> best;
    if (int rc = boot_run(ctx, dev, std::vector<int32_t>(members, members + m), (uint32_t)k, sm, std::vector<int32_t>(set_pos, set_pos + off), medoids, cluster, best, ms_kernel)) return rc;
    for (size_t i = 0; i < (size_t)n_sets * k; ++i) { best_inter[i] = best[2 * i]; best_union[i] = best[2 * i + 1]; }
    return MSNV_OK;
}

extern "C" int msnv_membership_stability_file(msnv_ctx *ctx, const char *dist_used_path, const char *clus_num_stability_path, const char *species, int32_t k,
                                              const char *out_dir, const msnv_membstab_opts *opts, int64_t result[8], double *ms_kernel) {
    clear_error();
    if (!ctx || !dist_used_path || !species || !out_dir) return fail(MSNV_EINVAL, "msnv_membership_stability_file: NULL argument");
    msnv_membstab_opts o;
    msnv_membstab_opts_default(&o);
    if (opts) o = *opts;
    if (o.reserved != 0 || o.boot_iters < 1 || o.boot_iters > 1024)
        return fail(MSNV_EINVAL, "msnv_membership_stability_file: boot_iters = %d, reserved = %d (1..1024 iterations, reserved 0)", o.boot_iters, o.reserved);
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    double ms = 0;
    std::vector<std::string> names;
    std::vector<double> d;
    if (int rc = read_dist(dist_used_path, names, d, true)) return rc;
    const uint32_t n = (uint32_t)names.size();
    if (names.size() < 10) {                                           // clustering.R:359: the stability is rated when nSamples >= 10
        if (result) { result[0] = MSNV_MEMBSTAB_NOT_RATED; result[1] = k; result[2] = n; }
        return MSNV_OK;
    }
    if (int rc = check_matrix(dist_used_path, (int64_t)names.size(), d.data())) return rc;
    if (k < 1 || k > (int32_t)CLUSTER_BOOT_MAX_K || (uint32_t)k >= n)
        return fail(MSNV_EDOMAIN, "msnv_membership_stability_file: k = %d with %u samples (1 <= k <= %u, k < samples)", k, n, CLUSTER_BOOT_MAX_K);
    int num_score = 0;
    if (clus_num_stability_path) {
        std::vector<double> prop;
        std::vector<int32_t> num;
        if (int rc = read_num_stability(clus_num_stability_path, prop, num)) return rc;
        num_score = stab_score(prop, num);
    }
    if (int rc = dev_set_device(ctx->device)) return rc;
    if (int rc = make_dir(out_dir)) return rc;

    // ---- the subsets of every proportion that can be clustered, in one batch
    const uint32_t K = (uint32_t)k, B = (uint32_t)o.boot_iters;
    const std::vector<SubsampleStep> steps = subsample_steps(n);
    std::vector<int32_t> members(n), set_pos, p;
    for (uint32_t i = 0; i < n; ++i) members[i] = (int32_t)i;
    std::vector<uint32_t> set_m;
    for (uint32_t pi = 0; pi < steps.size(); ++pi) {
        if (steps[pi].size <= K) continue;                             // pam stops at k >= n: rows of NA
        for (uint32_t b = 0; b < B; ++b) {
            permutation(o.seed, 1ull << 62 | (uint64_t)pi << 32 | b, n, p);
            set_m.push_back(steps[pi].size);
            set_pos.insert(set_pos.end(), p.begin(), p.begin() + steps[pi].size);
        }
    }
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, d.data(), n, ctx->stream)) return rc;
    std::vector<int32_t> medoids(K), clus(n), best;
    if (int rc = boot_run(ctx, dev, members, K, set_m, set_pos, medoids.data(), clus.data(), best, &ms)) return rc;

    // ---- per proportion and cluster: mean Jaccard, recovered / dissolved
    std::vector<MembRow> rows(steps.size() * K, MembRow{true, 0.0, 0.0});
    std::vector<double> jac(B);
    size_t t0 = 0;
    for (uint32_t pi = 0; pi < steps.size(); ++pi) {
        if (steps[pi].size <= K) continue;
        for (uint32_t j = 0; j < K; ++j) {
            uint32_t recovered = 0, dissolved = 0;
            for (uint32_t b = 0; b < B; ++b) {
                const int32_t *pair = &best[((t0 + b) * K + j) * 2];
                jac[b] = (double)pair[0] / (double)pair[1];
                recovered += jac[b] >= 0.75; dissolved += jac[b] <= 0.5;
            }
            rows[(size_t)pi * K + j] = MembRow{false, r_mean(jac.data(), B), (double)recovered / (double)dissolved};
        }
        t0 += B;
    }
    std::vector<uint32_t> sizes(K, 0);
    for (int32_t c : clus) ++sizes[c - 1];

    // ---- the files
    const std::string prefix = std::string(out_dir) + "/" + species + "_mann";
    std::string text = "clusterID\tnSamplesInCluster\tsubsampleProp\tclusterStabilityJaccardMean\tclusterStabilityPropRecover\n";
    for (uint32_t pi = 0; pi < steps.size(); ++pi)
        for (uint32_t j = 0; j < K; ++j) {
            const MembRow &r = rows[(size_t)pi * K + j];
            text += std::to_string(j + 1) + "\t" + std::to_string(sizes[j]) + "\t";
            r_double(steps[pi].prop, text);
            if (r.na) text += "\tNA\tNA\n";
            else { text.push_back('\t'); r_value(r.jaccard, text); text.push_back('\t'); r_value(r.recover, text); text.push_back('\n'); }
        }
    if (int rc = write_text(prefix + "_clusMembStability.tab", text)) return rc;
    int lowest = 3;
    text = std::string("name\tscore\nnumClusters\t") + SCORE_NAMES[num_score] + "\n";
    for (uint32_t j = 0; j < K; ++j) {
        const int sc = memb_score(steps, rows, K, j);
        lowest = std::min(lowest, sc);
        text += "clust" + std::to_string(j + 1) + "\t" + SCORE_NAMES[sc] + "\n";
    }
    if (int rc = write_text(prefix + "_stabilityAssessment.tab", text)) return rc;
    if (result) {
        result[0] = MSNV_MEMBSTAB_OK; result[1] = k; result[2] = n; result[3] = (int64_t)steps.size(); result[4] = (int64_t)set_m.size();
        result[5] = num_score; result[6] = lowest;
    }
    if (ms_kernel) *ms_kernel = ms;
    return MSNV_OK;
}
