// metasnv_amd/csrc/pcoa.cpp -- host side of subpopr's computePCoA (src/subpopr/R/clustering.R:120-126, :472-505; the kernels and their launches are
// pcoa_k.hip).
//
//   msnv_pcoa        ape::pcoa(correction = "none") of one distance matrix: eigenvalues, their shares and the first n_axes axes
//   msnv_pcoa_file   the stage: the matrix msnv_cluster_file read, its outliers removed by the same routine (cluster.cpp: remove_outliers), the
//                    ordination, and <species>_mann_pcoa_proj.tab with the cluster and the 10/90 proportion of every sample beside its two axes
// What is on the host: reading and writing, the checks, the outlier rule, the order of the n eigenvalues.  The centring, every rotation and the
// axes are on the device; there is no CPU fallback.
// Divergences: the eigenvector signs are ours, not LAPACK's; <species>_mann_pcoa_eig.tab is a file the reference does not write.
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "dataset.h"
#include "device.h"

namespace msnv {

// ---- what msnv_heatmap_file (hclust.cpp) shares with this file (device.h)
// A table as write.table(sep = '\t', quote = F) prints it: a header without a cell for the row names, then name + cells.  Returns the cell of column
// `column` per row name, as text.
int read_r_column(const std::string &path, const char *column, std::unordered_map<std::string, std::string> &cell) {
    std::string text;
    if (int rc = slurp(path, text)) return rc;
    std::vector<Span> lines, f;
    split_span(text.data(), text.data() + text.size(), '\n', lines);
    size_t col = 0, n_cols = 0;
    for (size_t l = 0; l < lines.size(); ++l) {
        const char *s = lines[l].first, *e = lines[l].second;
        if (e > s && e[-1] == '\r') --e;
        if (l && s == e) continue;
        split_span(s, e, '\t', f);
        if (l == 0) {
            n_cols = f.size();
            for (col = 0; col < n_cols; ++col) if (std::string(f[col].first, f[col].second) == column) break;
            if (col == n_cols) return fail(MSNV_EFORMAT, "%s: no column '%s'", path.c_str(), column);
            continue;
        }
        if (f.size() != n_cols + 1) return fail(MSNV_EFORMAT, "%s:%zu: %zu cells for %zu columns", path.c_str(), l + 1, f.size() - 1, n_cols);
        cell.emplace(std::string(f[0].first, f[0].second), std::string(f[col + 1].first, f[col + 1].second));
    }
    return MSNV_OK;
}

bool file_exists(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

}  // namespace msnv

using namespace msnv;

extern "C" int msnv_pcoa(msnv_ctx *ctx, int32_t n, const double *dist, int32_t n_axes, double *eig, double *rel_eig, double *axis_pct, double *vectors, int64_t info[8],
                         double *ms_kernel) {
    clear_error();
    if (!ctx || !dist || !eig || !rel_eig || !axis_pct || !vectors || !info) return fail(MSNV_EINVAL, "msnv_pcoa: NULL argument");
    if (ms_kernel) *ms_kernel = 0;
    if (int rc = check_matrix("msnv_pcoa", n, dist)) return rc;
    if (n_axes < 1 || n_axes > n) return fail(MSNV_EINVAL, "msnv_pcoa: %d axes of %d samples (1 <= n_axes <= n)", n_axes, n);
    if (int rc = dev_set_device(ctx->device)) return rc;
    return dev_pcoa("msnv_pcoa", dist, (uint32_t)n, (uint32_t)n_axes, ctx->stream, eig, rel_eig, axis_pct, vectors, info, ms_kernel);
}

extern "C" int msnv_pcoa_file(msnv_ctx *ctx, const char *dist_path, const char *dir, const char *species, int64_t result[8], double *ms_kernel) {
    clear_error();
    if (!ctx || !dist_path || !dir || !species) return fail(MSNV_EINVAL, "msnv_pcoa_file: NULL argument");
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    std::vector<std::string> names;
    std::vector<double> d;
    if (int rc = read_dist(dist_path, names, d)) return rc;
    const size_t n_all = names.size();
    if (int rc = check_matrix(dist_path, (int64_t)n_all, d.data())) return rc;
    const std::vector<int32_t> qc = remove_outliers(d, n_all);         // computeClusters hands computePCoA the matrix after outlier removal
    if (qc.size() < 2) return fail(MSNV_EDOMAIN, "%s: %zu samples left after outlier removal", dist_path, qc.size());
    const uint32_t n = (uint32_t)qc.size();
    const std::string prefix = std::string(dir) + "/" + species, comp_path = prefix + "_freq_composition.tab";
    std::unordered_map<std::string, std::string> clust, homog;
    if (int rc = read_r_column(prefix + "_mann_clustering.tab", "clust", clust)) return rc;
    if (file_exists(comp_path)) if (int rc = read_r_column(comp_path, "freq_data_sample_10_90", homog)) return rc;
    std::vector<std::string> homog_text(n, "NA");
    for (uint32_t a = 0; a < n; ++a) {
        auto it = homog.find(names[qc[a]]);
        if (it == homog.end() || it->second == "NA") continue;
        double v = NAN;
        if (it->second != "NaN" && !parse_finite(it->second.data(), it->second.data() + it->second.size(), v))
            return fail(MSNV_EFORMAT, "%s: the proportion of sample %s is '%s'", comp_path.c_str(), names[qc[a]].c_str(), it->second.c_str());
        homog_text[a].clear();
        r_double(v, homog_text[a]);
    }
    if (int rc = dev_set_device(ctx->device)) return rc;

    std::vector<double> sub((size_t)n * n), eig(n), rel(n), pct(n), axes((size_t)n * 2);
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) sub[(size_t)a * n + b] = d[(size_t)qc[a] * n_all + qc[b]];
    int64_t info[8];
    if (int rc = dev_pcoa(species, sub.data(), n, 2, ctx->stream, eig.data(), rel.data(), pct.data(), axes.data(), info, ms_kernel)) return rc;

    // ---- the files: ours first (the numbers R keeps for the axis labels), then the reference's, unless fewer than two axes came out
    std::string text = "Eigenvalues\tRelative_eig\taxisPercent\n";
    for (uint32_t a = 0; a < n; ++a) {
        text += std::to_string(a + 1);
        for (const double v : {eig[a], rel[a], pct[a]}) { text.push_back('\t'); r_value(v, text); }
        text.push_back('\n');
    }
    if (int rc = write_text(prefix + "_mann_pcoa_eig.tab", text)) return rc;
    if (info[0] == MSNV_PCOA_OK) {
        text = "Axis.1\tAxis.2\tpropFreqHomog\tclust\n";
        for (uint32_t a = 0; a < n; ++a) {
            const std::string &name = names[qc[a]];
            text += name;
            for (int c = 0; c < 2; ++c) { text.push_back('\t'); r_value(axes[(size_t)a * 2 + c], text); }
            auto it = clust.find(name);
            text += "\t" + homog_text[a] + "\t" + (it == clust.end() ? std::string("NA") : it->second) + "\n";
        }
        if (int rc = write_text(prefix + "_mann_pcoa_proj.tab", text)) return rc;
    }
    if (result) {
        for (int i = 0; i < 5; ++i) result[i] = info[i];
        result[5] = n; result[6] = (int64_t)(n_all - n);
    }
    return MSNV_OK;
}
