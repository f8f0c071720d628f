// metasnv_amd/csrc/genecorr.cpp -- host side of subpopr's correlateSubpopProfileWithGeneProfiles
// (src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R; the kernels are genecorr_k.hip).
//
//   msnv_gene_corr         the array form: cluster vectors x gene rows -> Spearman rho, Pearson r of the logs, valid flags (:141-153)
//   msnv_corr_stats        cor.test's derived columns and p.adjust(method = "BH") for one table (:153, :200)
//   msnv_gene_corr_files   the whole function: reads <species>_allClust_relativeAbund.tab and the gene-family table, keeps the clusters
//                          seen in >= 3 samples (:24-29), the samples both tables hold (:38-78), the genes present in them (:81-93), runs
//                          the two above, applies selectSubspeciesSpecificGenes (:238-303) and writes the four tables (:201, :210-211)
// Divergences: a cell that is NA, empty or not a number is refused with MSNV_EFORMAT (R drops such pairs);
// labels sort in byte order (R sorts in its locale); numbers are printed as the shortest digits that read back, exponent unpadded.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "dataset.h"
#include "device.h"

namespace msnv {

namespace {

inline Span trimmed(Span x) {                                          // readr's trim_ws
    while (x.first < x.second && (*x.first == ' ' || *x.first == '\r')) ++x.first;
    while (x.second > x.first && (x.second[-1] == ' ' || x.second[-1] == '\r')) --x.second;
    return x;
}

// a finite number, nothing else (NA, the empty field, nan and inf are refused)
inline bool parse_cell(Span x, double &v) {
    x = trimmed(x);
    return parse_finite(x.first, x.second, v);
}

// lines of a text, without their newline (and without a carriage return before it)
template <class F> int each_line(const std::string &text, F f) {
    const char *p = text.data(), *end = p + text.size();
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl : end, *next = nl ? nl + 1 : end;
        if (le > p && le[-1] == '\r') --le;
        if (int rc = f(p, le)) return rc;
        p = next;
    }
    return MSNV_OK;
}

// the shortest digits that read back; the exponent as readr writes it (1e-8, not 1e-08); NA, Inf, -Inf as R writes them
void r_number(double v, std::string &out) {
    if (v != v) { out += "NA"; return; }
    if (std::isinf(v)) { out += v > 0 ? "Inf" : "-Inf"; return; }
    const size_t at = out.size();
    py_repr(v, out);
    const size_t e = out.find('e', at);
    if (e != std::string::npos) {
        size_t d = e + 1;
        if (d < out.size() && (out[d] == '-' || out[d] == '+')) ++d;
        size_t z = d;
        while (z + 1 < out.size() && out[z] == '0') ++z;
        out.erase(d, z - d);
    }
}

struct Table {                                                         // one method's rows, cluster-major
    std::vector<uint32_t> clust; std::vector<uint64_t> gene;
    std::vector<double> est, stat, p, lo, hi, q;
};

// The text of a table is built whole and handed to write_text: about 120 bytes per row, next to the gene table's text and matrix that the stage holds anyway
int write_table(const std::string &path, bool pearson, const Table &t, const std::vector<std::string> &labels, const std::vector<std::string> &gene_names, int32_t n_obs) {
    std::string text = pearson ? "geneFamily\tcluster\tstatistic\tp.value\testimate\tnull.value\talternative\tmethod\tconf.int\tconf.int.low\tconf.int.high\tnObs\tq.valueBH\n"
                               : "geneFamily\tcluster\tstatistic\tp.value\testimate\tnull.value\talternative\tmethod\tnObs\tq.valueBH\n";
    const std::string nobs = std::to_string(n_obs);
    for (size_t i = 0; i < t.est.size(); ++i) {
        text += gene_names[t.gene[i]]; text.push_back('\t'); text += labels[t.clust[i]]; text.push_back('\t');
        r_number(t.stat[i], text); text.push_back('\t');
        r_number(t.p[i], text); text.push_back('\t');
        r_number(t.est[i], text);
        text += pearson ? "\t0\ttwo.sided\tpearson\tFALSE\t" : "\t0\ttwo.sided\tspearman\t";
        if (pearson) { r_number(t.lo[i], text); text.push_back('\t'); r_number(t.hi[i], text); text.push_back('\t'); }
        text += nobs; text.push_back('\t');
        r_number(t.q[i], text); text.push_back('\n');
    }
    return write_text(path, text);
}

struct Group { std::string gene; uint32_t clust; bool corr, not_corr; };

int write_groups(const std::string &path, const std::vector<Group> &rows, const std::vector<std::string> &labels) {
    std::string text = "geneFamily\tcluster\tgeneIsCorrelated\tgeneIsNotCorrelated\n";
    for (const Group &g : rows) {
        text += g.gene; text.push_back('\t'); text += labels[g.clust];
        text += g.corr ? "\tTRUE" : "\tFALSE"; text += g.not_corr ? "\tTRUE\n" : "\tFALSE\n";
    }
    return write_text(path, text);
}

std::string first_three(const std::vector<std::string> &v) {
    std::string s;
    for (size_t i = 0; i < v.size() && i < 3; ++i) { if (i) s += ", "; s += v[i]; }
    return s;
}

int check_samples(int32_t n_samples) {
    if (n_samples < 3) return fail(MSNV_EDOMAIN, "gene correlation: %d samples; cor.test stops below 3 observations", n_samples);
    if ((uint32_t)n_samples > GENECORR_MAX_SAMPLES)
        return fail(MSNV_EDOMAIN, "gene correlation: %d samples; one workgroup ranks a row in LDS and holds at most %u", n_samples, GENECORR_MAX_SAMPLES);
    return MSNV_OK;
}

}  // namespace
}  // namespace msnv

using namespace msnv;

extern "C" int msnv_gene_corr(msnv_ctx *ctx, int32_t n_clusters, int64_t n_genes, int32_t n_samples, const double *clust, const double *genes, double *rho,
                              double *r, uint8_t *valid, double *pseudocount, double *ms_kernel) {
    clear_error();
    if (!ctx || !clust || !genes || !rho || !r || !valid || n_clusters <= 0 || n_genes < 0) return fail(MSNV_EINVAL, "msnv_gene_corr: NULL argument or a count below its minimum");
    if (int rc = check_samples(n_samples)) return rc;
    if (int rc = dev_set_device(ctx->device)) return rc;
    if (ms_kernel) *ms_kernel = 0;
    if (n_genes == 0) return fail(MSNV_EDOMAIN, "gene correlation: no gene row (the reference's pseudocount is the smallest cell above 0 / 1000)");
    return dev_gene_corr((uint32_t)n_clusters, (uint64_t)n_genes, (uint32_t)n_samples, clust, genes, ctx->stream, rho, r, valid, pseudocount, ms_kernel);
}

extern "C" int msnv_corr_stats(msnv_ctx *ctx, int32_t method, uint64_t n, const double *estimate, const int32_t *n_obs, double *statistic, double *p_value,
                               double *conf_low, double *conf_high, double *q_value) {
    clear_error();
    if (!ctx || (n && (!estimate || !n_obs || !statistic || !p_value || !q_value))) return fail(MSNV_EINVAL, "msnv_corr_stats: NULL argument");
    if (method != MSNV_CORR_PEARSON && method != MSNV_CORR_SPEARMAN) return fail(MSNV_EINVAL, "msnv_corr_stats: method %d", method);
    if (n > 0x7fffffffull) return fail(MSNV_EDOMAIN, "msnv_corr_stats: %llu rows (at most 2^31 - 1)", (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i) {
        if (n_obs[i] < 3) return fail(MSNV_EDOMAIN, "msnv_corr_stats: row %llu has %d observations; cor.test stops below 3", (unsigned long long)i, n_obs[i]);
        if (!(estimate[i] >= -1.0 && estimate[i] <= 1.0)) return fail(MSNV_EDOMAIN, "msnv_corr_stats: row %llu: the estimate is not in [-1, 1]", (unsigned long long)i);
    }
    if (int rc = dev_set_device(ctx->device)) return rc;
    return dev_corr_stats(method, n, estimate, n_obs, ctx->stream, statistic, p_value, conf_low, conf_high, q_value);
}

extern "C" int msnv_gene_corr_files(msnv_ctx *ctx, const char *clust_abund_path, const char *gene_abund_path, const char *sample_suffix, const char *out_prefix,
                                    uint64_t counts[4]) {
    clear_error();
    if (!ctx || !clust_abund_path || !gene_abund_path || !out_prefix) return fail(MSNV_EINVAL, "msnv_gene_corr_files: NULL argument");
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (int rc = dev_set_device(ctx->device)) return rc;
    std::vector<Span> f;

    // ---- the cluster abundances: write.table's layout, the header one field short (:21-29)
    std::string ctext;
    if (int rc = slurp(clust_abund_path, ctext)) return rc;
    std::vector<std::string> cnames, csamples;
    std::vector<double> cab;                                           // [sample][K]
    uint64_t lineno = 0;
    if (int rc = each_line(ctext, [&](const char *s, const char *e) -> int {
            ++lineno;
            if (s == e) return MSNV_OK;
            split_span(s, e, '\t', f);
            if (lineno == 1) { for (Span x : f) cnames.emplace_back(x.first, x.second); return MSNV_OK; }
            if (f.size() != cnames.size() + 1) return fail(MSNV_EFORMAT, "%s:%llu: %zu fields, the header names %zu clusters (expected the sample name and one value per cluster)", clust_abund_path, (unsigned long long)lineno, f.size(), cnames.size());
            csamples.emplace_back(f[0].first, f[0].second);
            for (size_t k = 1; k < f.size(); ++k) {
                double v;
                if (!parse_cell(f[k], v)) return fail(MSNV_EFORMAT, "%s:%llu: '%s' is not a number (NA and empty cells are refused)", clust_abund_path, (unsigned long long)lineno, std::string(f[k].first, f[k].second).c_str());
                cab.push_back(v);
            }
            return MSNV_OK;
        })) return rc;
    const size_t K_all = cnames.size();
    std::vector<std::pair<std::string, size_t>> kept;                  // label, column
    for (size_t k = 0; k < K_all; ++k) {
        size_t seen = 0;
        for (size_t s = 0; s < csamples.size(); ++s) seen += cab[s * K_all + k] > 0;
        if (seen >= 3) kept.emplace_back(cnames[k][0] == 'X' ? cnames[k].substr(1) : cnames[k], k);
    }
    if (kept.empty()) return MSNV_OK;                                  // "No subspecies seen in >= 3 samples" (:31-34)
    std::sort(kept.begin(), kept.end());
    const size_t K = kept.size(), K1 = K + 1;
    std::unordered_map<std::string, size_t> sub_sample;                // samples with abundance > 0 in a kept cluster -> row
    std::vector<std::string> sub_names;
    for (size_t s = 0; s < csamples.size(); ++s) {
        bool any = false;
        for (auto &kc : kept) any |= cab[s * K_all + kc.second] > 0;
        if (any && sub_sample.emplace(csamples[s], s).second) sub_names.push_back(csamples[s]);
    }

    // ---- the gene-family table: '#' lines skipped, header id + samples (:42-93)
    std::string gtext;
    if (int rc = slurp(gene_abund_path, gtext)) return rc;
    std::vector<std::string> gcols, gene_names;
    std::vector<size_t> use_col, use_row;                              // gene-table column (0-based among the samples) -> cluster-table row
    std::vector<double> genes, cells;
    bool have_header = false;
    lineno = 0;
    int rc = each_line(gtext, [&](const char *s, const char *e) -> int {
        ++lineno;
        if (s == e || *s == '#') return MSNV_OK;
        split_span(s, e, '\t', f);
        if (!have_header) {
            have_header = true;
            for (size_t k = 1; k < f.size(); ++k) { Span x = trimmed(f[k]); gcols.emplace_back(x.first, x.second); }
            for (int attempt = 0; attempt < 2 && use_col.empty(); ++attempt) {
                if (attempt == 1 && !sample_suffix) break;
                std::unordered_set<std::string> taken;
                for (size_t k = 0; k < gcols.size(); ++k) {
                    const std::string name = attempt ? gcols[k] + sample_suffix : gcols[k];
                    auto it = sub_sample.find(name);
                    if (it != sub_sample.end() && taken.insert(name).second) { use_col.push_back(k); use_row.push_back(it->second); }
                }
            }
            if (use_col.empty())
                return fail(MSNV_EDOMAIN, "No overlapping sample IDs between clustering and gene family abundance profiles. Are IDs formatted differently? "
                            "Example clustering sample IDs: %s. Example gene family sample IDs: %s", first_three(sub_names).c_str(), first_three(gcols).c_str());
            return check_samples((int32_t)std::min<size_t>(use_col.size(), 0x7fffffff));
        }
        if (f.size() != gcols.size() + 1) return fail(MSNV_EFORMAT, "%s:%llu: %zu fields, the header has %zu", gene_abund_path, (unsigned long long)lineno, f.size(), gcols.size() + 1);
        cells.resize(gcols.size());
        for (size_t k = 0; k < gcols.size(); ++k)
            if (!parse_cell(f[k + 1], cells[k])) return fail(MSNV_EFORMAT, "%s:%llu: '%s' is not a number (NA and empty cells are refused)", gene_abund_path, (unsigned long long)lineno, std::string(f[k + 1].first, f[k + 1].second).c_str());
        double sum = 0;
        for (size_t c : use_col) sum += cells[c];
        if (!(sum > 0)) return MSNV_OK;                                // rowSums(...) > 0 (:85)
        Span id = trimmed(f[0]);
        gene_names.emplace_back(id.first, id.second);
        for (size_t c : use_col) genes.push_back(cells[c]);
        return MSNV_OK;
    });
    if (rc) return rc;
    if (!have_header) return fail(MSNV_EFORMAT, "%s: no header line", gene_abund_path);
    const size_t S = use_col.size(), G = gene_names.size();
    if (G == 0) return fail(MSNV_EDOMAIN, "%s: no gene family with abundance above 0 in the %zu samples used", gene_abund_path, S);

    // ---- the cluster vectors over the used samples, 0 where the cell was not > 0; the species row "-1" = their column sums (:126-139)
    std::vector<std::string> labels;
    for (auto &kc : kept) labels.push_back(kc.first);
    labels.push_back("-1");
    std::vector<double> clust(K1 * S, 0.0);
    for (size_t k = 0; k < K; ++k)
        for (size_t s = 0; s < S; ++s) {
            const double v = cab[use_row[s] * K_all + kept[k].second];
            clust[k * S + s] = v > 0 ? v : 0.0;
            clust[K * S + s] += clust[k * S + s];
        }

    std::vector<double> rho(K1 * G), r(K1 * G);
    std::vector<uint8_t> valid(K1 * G);
    double pc = 0, ms = 0;
    if ((rc = dev_gene_corr((uint32_t)K1, G, (uint32_t)S, clust.data(), genes.data(), ctx->stream, rho.data(), r.data(), valid.data(), &pc, &ms))) return rc;

    // ---- one table per method, cluster-major, genes in file order (:172-203)
    Table tab[2];                                                      // [0] pearson [1] spearman
    for (int m = 0; m < 2; ++m) {
        Table &t = tab[m];
        for (size_t c = 0; c < K1; ++c)
            for (size_t g = 0; g < G; ++g)
                if (valid[c * G + g]) { t.clust.push_back((uint32_t)c); t.gene.push_back(g); t.est.push_back(m ? rho[c * G + g] : r[c * G + g]); }
        const size_t n = t.est.size();
        t.stat.resize(n); t.p.resize(n); t.q.resize(n); t.lo.resize(n); t.hi.resize(n);
        std::vector<int32_t> nobs(n, (int32_t)S);
        if ((rc = dev_corr_stats(m, n, t.est.data(), nobs.data(), ctx->stream, t.stat.data(), t.p.data(), t.lo.data(), t.hi.data(), t.q.data()))) return rc;
    }
    const std::string prefix = out_prefix;
    if ((rc = write_table(prefix + "-spearman.tsv", false, tab[1], labels, gene_names, (int32_t)S))) return rc;
    if ((rc = write_table(prefix + "-pearson.tsv", true, tab[0], labels, gene_names, (int32_t)S))) return rc;

    // ---- selectSubspeciesSpecificGenes with its defaults (:238-303).  A (gene, cluster) group holds its pearson and its spearman row: both
    // exist or neither does (the valid flag is the methods' common one), and both tables list the groups in the same order.
    const double min_obs = 10, cutoff = 0.05, max_bad = 0.2, min_p = 0.8, min_s = 0.6;
    std::map<std::string, std::vector<Group>> by_gene;                 // byte order of the gene name; clusters in table order within it
    for (size_t i = 0; i < tab[0].est.size(); ++i) {
        const double rp = tab[0].est[i], rs = tab[1].est[i];
        Group g;
        g.gene = gene_names[tab[0].gene[i]]; g.clust = tab[0].clust[i];
        g.corr = rp >= min_p && tab[0].q[i] < cutoff && rs >= min_s && tab[1].q[i] < cutoff && (double)S >= min_obs;
        g.not_corr = rp < max_bad && rs < max_bad;
        by_gene[g.gene].push_back(g);
    }
    std::vector<Group> species_rows, cluster_rows;
    std::set<std::string> species_genes, specific;
    for (auto &kv : by_gene)
        for (const Group &g : kv.second)
            if (g.clust == K && g.corr) { species_rows.push_back(g); species_genes.insert(g.gene); }
    for (auto &kv : by_gene) {
        std::vector<Group> gs;
        for (Group g : kv.second) if (g.clust != K) { if (species_genes.count(g.gene)) g.corr = false; gs.push_back(g); }
        size_t n_corr = 0, n_not = 0;
        for (const Group &g : gs) { n_corr += g.corr; n_not += g.not_corr; }
        if (n_corr < 1 || n_not < 1) continue;
        for (const Group &g : gs) if (g.corr != g.not_corr) { cluster_rows.push_back(g); specific.insert(g.gene); }
    }
    if ((rc = write_groups(prefix + "-clusterSpecificGenes.tsv", cluster_rows, labels))) return rc;
    if ((rc = write_groups(prefix + "-speciesSpecificGenes.tsv", species_rows, labels))) return rc;
    if (counts) { counts[0] = K; counts[1] = G; counts[2] = S; counts[3] = specific.size(); }
    return MSNV_OK;
}
