// metasnv_amd/csrc/snvfreq.cpp -- host side of the numbers behind subpopr's SNV-frequency plots (src/subpopr/R/snvFreqPlot.R:1-113, drawn for every
// species by defineSubpopulations, profileSubpops.R:152-158; the kernel and its launch are snvfreq_k.hip).
//
//   msnv_freq_curves     the counts of a table on the percent scale: per sample, cells <= k and >= 100 - k for k = 0..49, covered, outside a band
//   msnv_freq_bands      the three fixed bands of computeSnvFreqStats on the same arrays (msnv_freq_bands_k, cluster_k.hip): what msnv_cluster_file counts
//   msnv_snvfreq_file    the stage: reads <species>.filtered.freq on metaSNV's [0, 1] scale, counts on the device, writes the two tables
// What is on the host: reading and writing, the two thresholds as R computes them in double, one division per proportion and one addition per
// propPass.  Every cell is looked at on the device; there is no CPU fallback.
// Divergences: a cell outside [0, 100] is refused where R would count it; the two files are ours, the reference keeps these
// numbers as pixels; the histogram's bins are not written.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "dataset.h"
#include "device.h"

namespace msnv {

// computeSnvFreqStatsThreshold's band of maxPropReadsNonHomog (clustering.R:43-51, computeSnvFreqStats.R:31-46), in double as R computes it; shared
// with msnv_cluster_file_ex (device.h)
void strict_band(double max_prop_reads_non_homog, double &lo, double &hi) {
    const double h = max_prop_reads_non_homog > 0.5 ? 1.0 - max_prop_reads_non_homog : max_prop_reads_non_homog;      // clustering.R:43-44
    const double c = h * 100.0;
    hi = std::max(100.0 - c, c); lo = std::min(100.0 - c, c);
}

namespace {

struct Thresholds {
    int32_t match = 0;                                                 // the cutoffIndex (1..50) equal to maxPropReadsNonHomog * 100 + 1 in double, or 0
    double lo = 0, hi = 0;                                             // computeSnvFreqStatsThreshold's band
};

Thresholds thresholds(double max_prop_reads_non_homog) {
    Thresholds t;
    const double index = max_prop_reads_non_homog * 100.0 + 1.0;      // snvFreqPlot.R:6, :13: two roundings
    for (int32_t k = 1; k <= 50; ++k)
        if ((double)k == index) t.match = k;
    strict_band(max_prop_reads_non_homog, t.lo, t.hi);
    return t;
}

int check_opts(const char *who, const msnv_snvfreq_opts &o) {
    if (!(o.max_prop_reads_non_homog >= 0.0 && o.max_prop_reads_non_homog <= 1.0))
        return fail(MSNV_EINVAL, "%s: max_prop_reads_non_homog = %g (0 <= proportion <= 1)", who, o.max_prop_reads_non_homog);
    if (!(o.min_prop_homog_snv >= 0.0 && o.min_prop_homog_snv <= 1.0)) return fail(MSNV_EINVAL, "%s: min_prop_homog_snv = %g (0 <= proportion <= 1)", who, o.min_prop_homog_snv);
    if (o.reserved[0] || o.reserved[1]) return fail(MSNV_EINVAL, "%s: a reserved field is not 0", who);
    return MSNV_OK;
}

void put_logical(int v, std::string &out) { out += v < 0 ? "NA" : v ? "TRUE" : "FALSE"; }      // -1: NA

// The two tables of n_rows x names.size() cells from counts[sample][102]; result as msnv_snvfreq_file's
void tables(const std::vector<std::string> &names, uint64_t n_rows, const uint64_t *counts, const Thresholds &t, double min_prop_homog_snv, std::string &cutoffs,
            std::string &fixed, int64_t result[8]) {
    cutoffs = "cutoffIndex\tsampleID\tpropLow\tpropHigh\tpropSuffCov\tpropPass\tsampleUsedForMedoidDefn\n";
    fixed = "sampleID\tpropPass\tpropSuffCov\tsampleUsedForMedoidDefn\tpropHomogStrict\tselectedForDiscovery\n";
    int64_t n_used = 0, n_selected = 0, n_uncovered = 0;
    for (size_t s = 0; s < names.size(); ++s) {
        const uint64_t *c = counts + s * 102;
        const double n = (double)c[100], cov = n / (double)n_rows;
        if (c[100] == 0) ++n_uncovered;
        for (int32_t k = 1; k <= 50; ++k) {
            const double low = (double)c[k - 1] / n, high = (double)c[50 + k - 1] / n, pass = low + high;
            const int used = k != t.match || pass != pass ? -1 : pass > min_prop_homog_snv ? 1 : 0;
            cutoffs += std::to_string(k); cutoffs.push_back('\t'); cutoffs += names[s];
            for (const double v : {low, high, cov, pass}) { cutoffs.push_back('\t'); r_double(v, cutoffs); }
            cutoffs.push_back('\t'); put_logical(used, cutoffs); cutoffs.push_back('\n');
            if (k == t.match) {
                fixed += names[s];
                for (const double v : {pass, cov}) { fixed.push_back('\t'); r_double(v, fixed); }
                fixed.push_back('\t'); put_logical(used, fixed);
                n_used += used == 1;
            }
        }
        if (!t.match) fixed += names[s] + "\tNA\tNA\tNA";
        const double strict = (double)c[101] / n;
        const bool selected = strict >= min_prop_homog_snv;              // NaN: not selected
        fixed.push_back('\t'); r_double(strict, fixed);
        fixed.push_back('\t'); put_logical(selected ? 1 : 0, fixed); fixed.push_back('\n');
        n_selected += selected;
    }
    if (result) {
        result[0] = (int64_t)names.size(); result[1] = (int64_t)n_rows; result[2] = t.match;
        result[3] = n_used; result[4] = n_selected; result[5] = n_uncovered;
    }
}

int check_arrays(const char *who, const void *ctx, const double *rows, int64_t n_pos, int32_t n_samples, const void *counts) {
    if (!ctx || !counts || (n_pos > 0 && !rows)) return fail(MSNV_EINVAL, "%s: NULL argument", who);
    if (n_pos < 0 || n_samples < 1) return fail(MSNV_EINVAL, "%s: %lld rows of %d samples (rows >= 0, samples >= 1)", who, (long long)n_pos, n_samples);
    return MSNV_OK;
}

}  // namespace
}  // namespace msnv

using namespace msnv;

extern "C" void msnv_snvfreq_opts_default(msnv_snvfreq_opts *o) {
    if (!o) return;
    o->max_prop_reads_non_homog = 0.1; o->min_prop_homog_snv = 0.8;
    o->reserved[0] = o->reserved[1] = 0;
}

extern "C" void msnv_freq_curves_geometry(int32_t *rows_per_block, int32_t *columns_per_block) {
    if (rows_per_block) *rows_per_block = (int32_t)FREQ_CURVE_ROWS;
    if (columns_per_block) *columns_per_block = (int32_t)FREQ_CURVE_LANES;
}

extern "C" int msnv_freq_curves(msnv_ctx *ctx, const double *rows, int64_t n_pos, int32_t n_samples, double strict_lo, double strict_hi, uint64_t *counts,
                                double *ms_kernel) {
    clear_error();
    if (ms_kernel) *ms_kernel = 0;
    if (int rc = check_arrays("msnv_freq_curves", ctx, rows, n_pos, n_samples, counts)) return rc;
    if (strict_lo != strict_lo || strict_hi != strict_hi) return fail(MSNV_EINVAL, "msnv_freq_curves: the strict band is (%g, %g)", strict_lo, strict_hi);
    if (int rc = dev_set_device(ctx->device)) return rc;
    uint32_t outside = 0;
    if (int rc = dev_freq_curves(rows, (uint64_t)n_pos, (uint32_t)n_samples, strict_lo, strict_hi, ctx->stream, counts, &outside, ms_kernel)) return rc;
    if (outside) return fail(MSNV_EDOMAIN, "msnv_freq_curves: a cell is neither NaN nor within [0, 100]");
    return MSNV_OK;
}

extern "C" int msnv_freq_bands(msnv_ctx *ctx, const double *rows, int64_t n_pos, int32_t n_samples, uint64_t *counts, double *ms_kernel) {
    clear_error();
    if (ms_kernel) *ms_kernel = 0;
    if (int rc = check_arrays("msnv_freq_bands", ctx, rows, n_pos, n_samples, counts)) return rc;
    if (int rc = dev_set_device(ctx->device)) return rc;
    return dev_freq_bands(rows, (uint64_t)n_pos, (uint32_t)n_samples, ctx->stream, counts, ms_kernel);
}

extern "C" int msnv_snvfreq_file(msnv_ctx *ctx, const char *freq_path, const char *species, const char *out_dir, const msnv_snvfreq_opts *opts, int64_t result[8],
                                 double *ms_kernel) {
    clear_error();
    if (!ctx || !freq_path || !species || !out_dir) return fail(MSNV_EINVAL, "msnv_snvfreq_file: NULL argument");
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    msnv_snvfreq_opts o;
    msnv_snvfreq_opts_default(&o);
    if (opts) o = *opts;
    if (int rc = check_opts("msnv_snvfreq_file", o)) return rc;
    std::vector<std::string> names, labels;
    std::vector<double> rows;
    uint64_t n_pos = 0;
    if (int rc = read_freq(freq_path, names, &labels, rows, n_pos)) return rc;
    const size_t S = names.size();
    if (S == 0) return fail(MSNV_EFORMAT, "%s: no sample column", freq_path);
    if (S > 0x7fffffffull) return fail(MSNV_EDOMAIN, "%s: %zu sample columns", freq_path, S);
    for (uint64_t p = 0; p < n_pos; ++p)
        for (size_t s = 0; s < S; ++s) {
            double &x = rows[p * S + s];
            if (x > 1.0)                                               // profileSubpops.R:145-147
                return fail(MSNV_EDOMAIN, "%s: row '%s' holds %g. The max value in your SNV frequency file is > 1. Values are expected to be -1 or within [0 to 1]. "
                            "Are you using an old version of metaSNV?", freq_path, labels[p].c_str(), x);
            x *= 100.0;
        }
    if (int rc = dev_set_device(ctx->device)) return rc;
    const Thresholds t = thresholds(o.max_prop_reads_non_homog);
    std::vector<uint64_t> counts(S * 102);
    uint32_t outside = 0;
    if (int rc = dev_freq_curves(rows.data(), n_pos, (uint32_t)S, t.lo, t.hi, ctx->stream, counts.data(), &outside, ms_kernel)) return rc;
    if (outside) return fail(MSNV_EDOMAIN, "%s: a cell is neither -1 nor within [0 to 1]", freq_path);
    std::string cutoffs, fixed;
    tables(names, n_pos, counts.data(), t, o.min_prop_homog_snv, cutoffs, fixed, result);
    const std::string dir = std::string(out_dir) + "/snvFreqPlots", prefix = dir + "/" + species + "_snvFreq_";
    if (int rc = make_dir(out_dir)) return rc;
    if (int rc = make_dir(dir)) return rc;                             // getSnvFreqPlotDir, utils.R:49-55
    if (int rc = write_text(prefix + "cutoffs.tab", cutoffs)) return rc;
    return write_text(prefix + "fixed.tab", fixed);
}
