// metasnv_amd/csrc/genotype.cpp -- host side of subpopr's writeGenotypeFreqs -> computeUniquePosPerCluster (src/subpopr/R/writeGenotypeFreqs.R:2-112,
// :195-277; the kernel is genotype_k.hip).
//
//   msnv_genotype_rows    the rule on arrays: per table row, which clusters it genotypes and which of those are flipped
//   msnv_genotype_file    the stage: the clustering table and the *.filtered.freq table in, <species>_<cluster>_hap_positions.tab,
//                         <species>_hap_out.txt and <species>_hap_freq_{mean,median}.tab out
// What is on the host: reading and writing, the rows the kernel could not decide within its guard (redone in long double, R's rowMeans), and
// the per-sample mean / median over the selected rows (G x S cells, a compact copy).  The walk over the whole table is on the device; there
// is no CPU fallback.
// Everything here is restated from reading the R code; no R was run (unpinned).  Divergences (same section): the
// "cluster missing" ending is taken for any cluster without positions (R itself errors when it is the first); a single sample without
// classification is counted (R's rownames() of a dropped one-row matrix is NULL and it counts zero).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "dataset.h"
#include "device.h"

namespace msnv {

namespace {

// the column list of the kernel: columns in use in cluster order, ascending inside a cluster
int column_list(const char *who, int32_t S, const int32_t *clust, int32_t K, std::vector<uint32_t> &col, std::vector<uint32_t> &seg) {
    if (K < 2 || K > (int32_t)GENO_MAX_CLUSTERS) return fail(MSNV_EDOMAIN, "%s: %d clusters (2 to %u)", who, K, GENO_MAX_CLUSTERS);
    if (S < 1 || S > (int32_t)GENO_MAX_SAMPLES) return fail(MSNV_EDOMAIN, "%s: %d sample columns (1 to %u)", who, S, GENO_MAX_SAMPLES);
    seg.assign((size_t)K + 1, 0);
    for (int32_t s = 0; s < S; ++s) {
        if (clust[s] < 0 || clust[s] > K) return fail(MSNV_EDOMAIN, "%s: column %d is in cluster %d of %d", who, s, clust[s], K);
        if (clust[s]) ++seg[clust[s]];
    }
    for (int32_t k = 1; k <= K; ++k) {
        if (seg[k] == 0) return fail(MSNV_EDOMAIN, "%s: cluster %d has no column", who, k);
        seg[k] += seg[k - 1];
    }
    col.resize(seg[K]);
    std::vector<uint32_t> at(seg.begin(), seg.end() - 1);
    for (int32_t s = 0; s < S; ++s) if (clust[s]) col[at[clust[s] - 1]++] = (uint32_t)s;
    return MSNV_OK;
}

// One row by R's rule: rowMeans(na.rm = T) is a long double sum in column order over the count, rounded to double; the counts are integers
void host_row(const double *row, const std::vector<uint32_t> &col, const std::vector<uint32_t> &seg, uint32_t K, double threshold, uint32_t &sel, uint32_t &flip) {
    double mean[GENO_MAX_CLUSTERS];
    uint32_t na[GENO_MAX_CLUSTERS], lt[GENO_MAX_CLUSTERS], all_na = 0;
    for (uint32_t k = 0; k < K; ++k) {
        long double s = 0;
        na[k] = lt[k] = 0;
        for (uint32_t c = seg[k]; c < seg[k + 1]; ++c) {
            const double x = row[col[c]];
            if (x != x) ++na[k];
            else { s += x; lt[k] += x < 50.0; }
        }
        const uint32_t valid = seg[k + 1] - seg[k] - na[k];
        mean[k] = valid ? (double)(s / (long double)valid) : std::nan("");
        all_na += na[k];
    }
    sel = flip = 0;
    const uint32_t n_used = seg[K];
    for (uint32_t i = 0; i < K; ++i) {
        const uint32_t size = seg[i + 1] - seg[i], valid = size - na[i];
        if (!((double)na[i] / (double)size < 0.2) || !((double)(all_na - na[i]) / (double)(n_used - size) < 0.2)) continue;
        bool distinct = true;
        for (uint32_t j = 0; j < K && distinct; ++j) {
            if (j == i) continue;
            double f = std::fabs(mean[i] - mean[j]);
            if (f != f) f = 0.0;
            distinct = f > threshold;
        }
        if (!distinct) continue;
        sel |= 1u << i;
        if (lt[i] > valid - lt[i]) flip |= 1u << i;
    }
}

int genotype_rows(msnv_ctx *ctx, const char *who, uint64_t n_pos, int32_t S, const double *rows, const int32_t *clust, int32_t K, double threshold,
                  uint32_t *select_mask, uint32_t *flip_mask, uint64_t *n_rechecked, double *ms_kernel) {
    std::vector<uint32_t> col, seg;
    if (int rc = column_list(who, S, clust, K, col, seg)) return rc;
    if (!std::isfinite(threshold)) return fail(MSNV_EINVAL, "%s: the threshold is %g", who, threshold);
    if (int rc = dev_set_device(ctx->device)) return rc;
    std::vector<uint8_t> flag(n_pos);
    if (int rc = dev_genotype_rows(rows, n_pos, (uint32_t)S, col.data(), seg.data(), (uint32_t)K, threshold, ctx->stream, select_mask, flip_mask, flag.data(), ms_kernel)) return rc;
    uint64_t redone = 0;
    for (uint64_t p = 0; p < n_pos; ++p) {
        if (flag[p] & 2) return fail(MSNV_EDOMAIN, "%s: row %llu holds a cell outside [0, 100]", who, (unsigned long long)p);
        if (flag[p] & 1) { host_row(rows + p * (uint64_t)S, col, seg, (uint32_t)K, threshold, select_mask[p], flip_mask[p]); ++redone; }
    }
    if (n_rechecked) *n_rechecked = redone;
    return MSNV_OK;
}

// <species>_mann_clustering.tab as msnv_cluster_file writes it (write.table of a one-column data frame): "clust", then name<TAB>integer
int read_clustering(const char *path, std::unordered_map<std::string, int64_t> &id_of) {
    FILE *in = fopen(path, "r");
    if (!in) return fail(MSNV_EIO, "Cannot open %s: %s", path, strerror(errno));
    char *line = nullptr; size_t cap = 0; ssize_t len;
    uint64_t lineno = 0;
    int rc = MSNV_OK;
    while (rc == MSNV_OK && (len = getline(&line, &cap, in)) >= 0) {
        ++lineno;
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (lineno == 1) { if (strcmp(line, "clust") != 0) rc = fail(MSNV_EFORMAT, "%s:1: the header is '%s', not 'clust'", path, line); continue; }
        if (len == 0) continue;
        const char *t = (const char *)memchr(line, '\t', (size_t)len);
        if (!t || t == line || memchr(t + 1, '\t', (size_t)(line + len - t - 1))) { rc = fail(MSNV_EFORMAT, "%s:%llu: a row is a sample name and one cluster id", path, (unsigned long long)lineno); break; }
        int64_t id;
        if (!parse_small_int(t + 1, line + len, id)) { rc = fail(MSNV_EFORMAT, "%s:%llu: the cluster id '%s' is not an integer", path, (unsigned long long)lineno, t + 1); break; }
        if (!id_of.emplace(std::string((const char *)line, t), id).second) rc = fail(MSNV_EFORMAT, "%s:%llu: sample '%.*s' is listed twice", path, (unsigned long long)lineno, (int)(t - line), line);
    }
    free(line);
    fclose(in);
    return rc;
}

struct Cell { double v; bool na; };                                    // a median is NA, not NaN, when it has no value

void put_cell(const Cell &c, std::string &out) { if (c.na) out += "NA"; else r_double(c.v, out); }

}  // namespace
}  // namespace msnv

using namespace msnv;

extern "C" int msnv_genotype_rows(msnv_ctx *ctx, uint64_t n_pos, int32_t n_samples, const double *rows, const int32_t *clust, int32_t n_clusters, double threshold,
                                  uint32_t *select_mask, uint32_t *flip_mask, uint64_t *n_rechecked, double *ms_kernel) {
    clear_error();
    if (!ctx || !clust || (n_pos && (!rows || !select_mask || !flip_mask))) return fail(MSNV_EINVAL, "msnv_genotype_rows: NULL argument");
    if (n_rechecked) *n_rechecked = 0;
    if (ms_kernel) *ms_kernel = 0;
    return genotype_rows(ctx, "msnv_genotype_rows", n_pos, n_samples, rows, clust, n_clusters, threshold, select_mask, flip_mask, n_rechecked, ms_kernel);
}

extern "C" int msnv_genotype_file(msnv_ctx *ctx, const char *clustering_path, const char *freq_path, const char *species, const char *out_dir, double uniq_threshold,
                                  int64_t result[8], double *ms_kernel) {
    clear_error();
    if (!ctx || !clustering_path || !freq_path || !species || !out_dir) return fail(MSNV_EINVAL, "msnv_genotype_file: NULL argument");
    if (!(uniq_threshold > 0.0 && uniq_threshold < 1.0)) return fail(MSNV_EINVAL, "msnv_genotype_file: uniq_threshold = %g (0 < threshold < 1)", uniq_threshold);
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    std::unordered_map<std::string, int64_t> id_of;
    if (int rc = read_clustering(clustering_path, id_of)) return rc;
    std::vector<std::string> fnames, labels;
    std::vector<double> rows;
    uint64_t n_pos = 0;
    if (int rc = read_freq(freq_path, fnames, &labels, rows, n_pos)) return rc;
    const size_t S = fnames.size();
    if (S == 0) return fail(MSNV_EFORMAT, "%s: no sample column", freq_path);
    for (uint64_t p = 0; p < n_pos; ++p)
        for (size_t s = 0; s < S; ++s) {
            double &x = rows[p * S + s];
            if (x > 1.0) return fail(MSNV_EDOMAIN, "%s: row '%s' holds %g; values are -1 or within 0 to 1", freq_path, labels[p].c_str(), x);
            x *= 100.0;
        }
    if (int rc = dev_set_device(ctx->device)) return rc;

    // ---- the samples in use, in freq column order; clustIDs in order of first appearance
    std::vector<uint32_t> used;                                        // freq columns
    std::vector<int64_t> used_id, clust_ids;
    std::vector<int32_t> clust(S, 0);
    for (size_t s = 0; s < S; ++s) {
        auto it = id_of.find(fnames[s]);
        if (it == id_of.end()) continue;
        size_t k = std::find(clust_ids.begin(), clust_ids.end(), it->second) - clust_ids.begin();
        if (k == clust_ids.size()) clust_ids.push_back(it->second);
        if (k < GENO_MAX_CLUSTERS) clust[s] = (int32_t)k + 1;
        used.push_back((uint32_t)s); used_id.push_back(it->second);
        id_of.erase(it);                                               // a second freq column of the same name is not in use
    }
    const size_t K = clust_ids.size(), n_used = used.size();
    if (result) { result[1] = (int64_t)K; result[2] = (int64_t)n_used; result[3] = (int64_t)n_pos; }
    const std::string out = std::string(out_dir) + "/", sp = species, log_path = out + sp + "_hap_out.txt";
    if (int rc = make_dir(out_dir)) return rc;
    if (K <= 1) {
        if (result) result[0] = MSNV_GENOTYPE_SINGLE;
        return write_text(log_path, "Single cluster\n");
    }
    std::string log = "\n";
    const std::string no_positions = "No genotyping positions for  " + sp + "\n";
    if (*std::max_element(clust_ids.begin(), clust_ids.end()) < 1) {
        if (result) result[0] = MSNV_GENOTYPE_NO_POSITIONS;
        return write_text(log_path, log + no_positions);
    }

    // ---- computeUniquePosPerCluster: the table walk is the kernel's
    std::vector<uint32_t> sel(n_pos), flip(n_pos);
    uint64_t redone = 0;
    double ms = 0;
    if (int rc = genotype_rows(ctx, freq_path, n_pos, (int32_t)S, rows.data(), clust.data(), (int32_t)K, uniq_threshold * 100.0, sel.data(), flip.data(), &redone, &ms)) return rc;
    if (ms_kernel) *ms_kernel = ms;
    std::vector<std::vector<Cell>> mean_of(K), median_of(K);           // per cluster with positions: one cell per sample in use
    uint64_t n_positions = 0;
    size_t n_with = 0;
    std::vector<uint64_t> picked;
    std::vector<double> x;
    for (size_t k = 0; k < K; ++k) {
        picked.clear();
        for (uint64_t p = 0; p < n_pos; ++p) if (sel[p] >> k & 1) picked.push_back(p);
        if (picked.empty()) {
            log += "No unique genotyping positions for species " + sp + " cluster " + std::to_string(clust_ids[k]) + " (species has " + std::to_string(K) + " total clusters)\n";
            continue;
        }
        ++n_with; n_positions += picked.size();
        std::string text = "posId\tflip\n";
        for (size_t g = 0; g < picked.size(); ++g) {
            text += std::to_string(g + 1); text.push_back('\t'); text += labels[picked[g]];
            text += (flip[picked[g]] >> k & 1) ? "\tTRUE\n" : "\tFALSE\n";
        }
        if (int rc = write_text(out + sp + "_" + std::to_string(clust_ids[k]) + "_hap_positions.tab", text)) return rc;
        // apply(fDist_data, 2, mean / median, na.rm = T): flipped rows count as 100 - x
        for (size_t a = 0; a < n_used; ++a) {
            x.clear();
            for (uint64_t p : picked) {
                const double v = rows[p * S + used[a]];
                if (v == v) x.push_back((flip[p] >> k & 1) ? 100.0 - v : v);
            }
            if (x.empty()) { mean_of[k].push_back(Cell{std::nan(""), false}); median_of[k].push_back(Cell{0, true}); continue; }
            mean_of[k].push_back(Cell{r_mean(x.data(), x.size()), false});
            std::sort(x.begin(), x.end());
            const size_t h = x.size() / 2;
            median_of[k].push_back(Cell{x.size() & 1 ? x[h] : r_mean(x.data() + h - 1, 2), false});
        }
    }
    if (result) { result[4] = (int64_t)n_positions; result[5] = (int64_t)redone; }
    if (n_with == 0) {
        if (result) result[0] = MSNV_GENOTYPE_NO_POSITIONS;
        return write_text(log_path, log + no_positions);
    }
    if (n_with < K) {
        if (result) result[0] = MSNV_GENOTYPE_CLUSTER_MISSING;
        return write_text(log_path, log + "At least one cluster is missing genotyping positions for  " + sp + " . Aborting, but this could be fixed.\n");
    }

    // ---- coll: per sample one median per cluster; its row sum in long double, NA when a median is
    std::vector<uint32_t> bad, good;
    size_t n_without = 0;
    for (size_t a = 0; a < n_used; ++a) {
        long double s = 0;
        bool na = false;
        for (size_t k = 0; k < K; ++k) { na = na || median_of[k][a].na; s += median_of[k][a].v; }
        const double sum = (double)s;
        if (na) ++n_without;
        else if (sum > 120.0 || sum < 80.0) bad.push_back((uint32_t)a);
        else good.push_back((uint32_t)a);
    }
    if ((double)bad.size() > 0.15 * (double)n_used) {
        log += "Cutoff is bad\n";
        log += "In  " + std::to_string(bad.size()) + "  out of  " + std::to_string(n_used) +
               "  samples,  the summed abundance of all clusters per sample is >120% or < 80%,  based on the frequencies of the genotyping SNVs.\n";
        log += "Samples with incoherent cluster abundance measured based on genotyping SNVs: \n";
        for (uint32_t a : bad) { log += fnames[used[a]]; log.push_back('\n'); }
        if (result) result[0] = MSNV_GENOTYPE_CUTOFF_BAD;
        return write_text(log_path, log);
    }
    uint64_t n_corr = 0;
    for (uint32_t a : good) {
        size_t best = 0;
        for (size_t k = 1; k < K; ++k) if (median_of[k][a].v > median_of[best][a].v) best = k;       // which.max: the first largest
        n_corr += used_id[a] == (int64_t)best + 1;                     // the reference compares the cluster id with the column index
    }
    log += "Genotyping-based assignment of discovery samples to clusters was correct for " + std::to_string(n_corr) +
           " samples. Determined any cluster assignment from genotyping SNVs for " + std::to_string(good.size()) + " out of " + std::to_string(n_used) +
           " samples. Of those samples without assignments: " + std::to_string(bad.size()) + "  had incoherect cluster assignments and " + std::to_string(n_without) +
           " lacked coverage of genotyping SNVs.\n";
    if (int rc = write_text(log_path, log)) return rc;
    for (int which = 0; which < 2; ++which) {
        std::string text = "\ti\n";
        for (size_t k = 0; k < K; ++k)
            for (size_t a = 0; a < n_used; ++a) {
                text += fnames[used[a]]; text.push_back('\t');
                put_cell((which ? median_of : mean_of)[k][a], text);
                text.push_back('\t'); text += std::to_string(clust_ids[k]); text.push_back('\n');
            }
        if (int rc = write_text(out + sp + (which ? "_hap_freq_median.tab" : "_hap_freq_mean.tab"), text)) return rc;
    }
    if (result) { result[0] = MSNV_GENOTYPE_OK; result[6] = (int64_t)n_corr; result[7] = (int64_t)good.size(); }
    return MSNV_OK;
}
