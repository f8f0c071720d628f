// metasnv_amd/csrc/covext.cpp -- host side of qaCompute's -m / -p W / -x FILE (covext_k.hip computes the numbers): hands the device pass
// what it cannot know, keeps the results per accumulator row, and writes OUT (with Median_Cov), OUT.profile and OUT.specific exactly as
// qaCompute.cpp:100-123,173-186,215,237,249-260,344,437,604-615 formats them.  Only printf happens here.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <map>

#include "device.h"

namespace msnv {

// windows of a contig of L indices: the loop of qaCompute.cpp:175-182 prints one at every i = W, 2 W, ... < L, the trailing line (:183)
// exists unless (L - 1) % W == 0 -- none at all for L == 1
static uint64_t window_count(int64_t L, uint32_t W) {
    if (L < 2) return 0;
    return (uint64_t)(L - 1) / W + ((L - 1) % W != 0 ? 1 : 0);
}

int coverage_extras_run(msnv_dataset &ds, const msnv_cov_extras &what) {
    DeviceCols &d = *ds.dev;
    const size_t NC = ds.names.size(), n_rows = ds.cov_row_sample.size();
    if (what.window < 0) return fail(MSNV_EINVAL, "msnv_coverage_extras_run: window %d is negative", what.window);
    if (what.n_regions && (!what.region_contig || !what.region_start || !what.region_end)) return fail(MSNV_EINVAL, "msnv_coverage_extras_run: NULL region array");
    for (uint32_t i = 0; i < what.n_regions; ++i) {
        const int32_t c = what.region_contig[i], s = what.region_start[i], e = what.region_end[i];
        if (c < 0 || (size_t)c >= NC) return fail(MSNV_EINVAL, "msnv_coverage_extras_run: region %u names contig %d of %zu", i, c, NC);
        // the reference sums data[start .. end] of an array of L prefix sums (qaCompute.cpp:114-116): beyond it, it reads what is not one
        if (s < 0 || s > e || (int64_t)e >= ds.lengths[(size_t)c])
            return fail(MSNV_EDOMAIN, "region %u [%d, %d] does not lie inside contig %s of length %lld", i, s, e, ds.names[(size_t)c].c_str(), (long long)ds.lengths[(size_t)c]);
    }
    msnv_dataset::CovExtras &x = ds.covx;
    x = msnv_dataset::CovExtras{};
    x.have_median = what.want_median != 0;
    x.window = (uint32_t)what.window;
    x.reg_contig.assign(what.region_contig, what.region_contig + what.n_regions);
    x.reg_start.assign(what.region_start, what.region_start + what.n_regions);
    x.reg_end.assign(what.region_end, what.region_end + what.n_regions);

    CovxJob job;
    job.want_median = x.have_median; job.window = x.window; job.n_samples = (uint32_t)ds.samples.size();
    job.row_win_off.assign(n_rows + 1, 0);
    for (size_t r = 0; r < n_rows; ++r) job.row_win_off[r + 1] = job.row_win_off[r] + (x.window ? window_count(ds.lengths[ds.cov_row_contig[r]], x.window) : 0);
    if (x.have_median || x.window || what.n_regions) {
        // asking for none of the three launches nothing and reads nothing
        if (!ds.cov_row_scanned_ok) {
            ds.cov_row_scanned.assign(n_rows, 0);
            if (int rc = dev_coverage_scanned(d, ds.ctx->stream, ds.cov_row_scanned.data())) return rc;
            ds.cov_row_scanned_ok = true;
        }
        job.contig_tile_base.assign(ds.tile_base.begin(), ds.tile_base.end());
        job.contig_tile_base.resize(NC, UINT32_MAX);
        job.row_contig = ds.cov_row_contig;
        job.row_len.resize(n_rows);
        for (size_t r = 0; r < n_rows; ++r) job.row_len[r] = (uint64_t)ds.lengths[ds.cov_row_contig[r]];
        job.row_scanned.assign(ds.cov_row_scanned.begin(), ds.cov_row_scanned.end());
        std::vector<uint32_t> order(what.n_regions);
        for (uint32_t i = 0; i < what.n_regions; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) {
            return x.reg_contig[p] != x.reg_contig[q] ? x.reg_contig[p] < x.reg_contig[q] : x.reg_start[p] < x.reg_start[q]; });
        job.reg_off.assign(NC + 1, 0);
        for (uint32_t i : order) {
            const uint32_t c = (uint32_t)x.reg_contig[i], e = (uint32_t)x.reg_end[i];
            const bool first = job.reg_off[c + 1] == 0;
            job.regs.push_back(CovxRegion{(uint32_t)x.reg_start[i], e, first ? e : std::max(e, job.regs.back().max_end), i});
            job.reg_off[c + 1]++;
        }
        for (size_t c = 0; c < NC; ++c) job.reg_off[c + 1] += job.reg_off[c];
        if (int rc = dev_run_coverage_extras(d, job, ds.ctx->stream)) return rc;
    }
    else {
        job.row_median.assign(n_rows, 0);
    }
    x.row_median.swap(job.row_median);
    x.row_win_off.swap(job.row_win_off);
    x.win.swap(job.win);
    x.reg_sum.swap(job.reg_sum);
    x.reg_sum.resize(ds.samples.size() * (size_t)what.n_regions, 0);
    x.n_launches = job.n_launches;
    x.valid = true;
    return MSNV_OK;
}

// the row of (sample, contig), or SIZE_MAX: rows are sorted by contig inside a sample
static size_t row_of(const msnv_dataset &ds, size_t sample, uint32_t contig) {
    const auto lo = ds.cov_row_contig.begin() + (std::ptrdiff_t)ds.cov_row_start[sample], hi = ds.cov_row_contig.begin() + (std::ptrdiff_t)ds.cov_row_start[sample + 1];
    const auto it = std::lower_bound(lo, hi, contig);
    return it != hi && *it == contig ? (size_t)(it - ds.cov_row_contig.begin()) : SIZE_MAX;
}

int coverage_window_count(const msnv_dataset &ds, uint64_t *n) {
    *n = 0;
    if (ds.covx.window) for (size_t c = 0; c < ds.names.size(); ++c) *n += window_count(ds.lengths[c], ds.covx.window);
    return MSNV_OK;
}

int coverage_window_sums(const msnv_dataset &ds, int sample, uint64_t *out) {
    const msnv_dataset::CovExtras &x = ds.covx;
    if (!x.window) return MSNV_OK;
    for (size_t c = 0; c < ds.names.size(); ++c) {
        const uint64_t n = window_count(ds.lengths[c], x.window);
        const size_t r = row_of(ds, (size_t)sample, (uint32_t)c);
        if (r == SIZE_MAX) memset(out, 0, n * sizeof(uint64_t));
        else memcpy(out, x.win.data() + x.row_win_off[r], n * sizeof(uint64_t));
        out += n;
    }
    return MSNV_OK;
}

static int write_profile(const msnv_dataset &ds, int sample, const char *path) {
    const msnv_dataset::CovExtras &x = ds.covx;
    if (!x.window) return fail(MSNV_EINVAL, "no window sums: msnv_coverage_extras_run was not asked for a profile");
    FILE *f = fopen(path, "wt");
    if (!f) return fail(MSNV_EIO, "qaCompute: Unable to create profile output file %s", path);
    const int W = (int)x.window;
    for (size_t c = 0; c < ds.names.size(); ++c) {
        const int L = (int)ds.lengths[c];
        const size_t r = row_of(ds, (size_t)sample, (uint32_t)c);
        const uint64_t *sum = r == SIZE_MAX ? nullptr : x.win.data() + x.row_win_off[r];
        const char *name = ds.names[c].c_str();
        if (L < 2) continue;
        const int full = (L - 1) / W;
        // the divisor of a full window is W, also for the first, which holds W + 1 values (qaCompute.cpp:174-181)
        for (int k = 0; k < full; ++k) fprintf(f, "%s\t%d\t%d\t%4.5f\n", name, k * W + 1, (k + 1) * W, sum ? (double)sum[k] / W : 0.0);
        if ((L - 1) % W != 0) {                                                           // :183-185; printSkipped :258-260 prints 0.0 itself
            const int rest = L % W;
            double v = 0.0;
            if (sum) {
                // rest == 0: the reference divides by zero; x86-64 gives inf for a sum that is not zero and the negative quiet NaN for 0 / 0
                if (rest) v = (double)sum[full] / rest;
                else v = sum[full] ? HUGE_VAL : std::copysign(std::nan(""), -1.0);
            }
            fprintf(f, "%s\t%d\t%d\t%4.5f\n", name, L - rest + 1, L, v);
        }
    }
    if (fclose(f) != 0) return fail(MSNV_EIO, "write error on %s", path);
    return MSNV_OK;
}

static int write_specific(const msnv_dataset &ds, int sample, const char *path, const msnv_cov_region *regions, uint32_t n_regions) {
    const msnv_dataset::CovExtras &x = ds.covx;
    std::map<std::string, uint32_t> contig_of;
    for (size_t c = 0; c < ds.names.size(); ++c) contig_of.emplace(ds.names[c], (uint32_t)c);       // (the first of equal names, as a header lookup finds it)
    // the lines that name a header contig are, in order, the regions the device pass summed
    std::vector<uint32_t> run_id(n_regions, UINT32_MAX);
    std::map<std::string, std::vector<uint32_t>> by_name;                                           // qaCompute's iMap (:59,347): byte-wise name order
    uint32_t k = 0;
    for (uint32_t i = 0; i < n_regions; ++i) {
        if (!regions[i].contig || !regions[i].alias) return fail(MSNV_EINVAL, "msnv_write_coverage_ex: region %u has a NULL name", i);
        by_name[regions[i].contig].push_back(i);
        const auto it = contig_of.find(regions[i].contig);
        if (it == contig_of.end()) continue;
        if (k >= x.reg_contig.size() || (uint32_t)x.reg_contig[k] != it->second || x.reg_start[k] != regions[i].start || x.reg_end[k] != regions[i].end)
            return fail(MSNV_EINVAL, "msnv_write_coverage_ex: region %u (%s %d %d) is not region %u of the last msnv_coverage_extras_run", i, regions[i].contig,
                        regions[i].start, regions[i].end, k);
        run_id[i] = k++;
    }
    if (k != x.reg_contig.size()) return fail(MSNV_EINVAL, "msnv_write_coverage_ex: %u regions name a header contig, the last msnv_coverage_extras_run summed %zu", k, x.reg_contig.size());
    FILE *f = fopen(path, "wt");
    if (!f) return fail(MSNV_EIO, "qaCompute: Unable to create specific output file %s", path);
    const uint64_t *sums = x.reg_sum.data() + (size_t)sample * x.reg_contig.size();
    // contigs the sample has coverage on, in header order, each with its intervals in file order (specific_print_cov, :100-123) ...
    for (uint64_t r = ds.cov_row_start[(size_t)sample]; r < ds.cov_row_start[(size_t)sample + 1]; ++r) {
        const auto it = by_name.find(ds.names[ds.cov_row_contig[(size_t)r]]);
        if (it == by_name.end()) continue;
        for (uint32_t i : it->second) fprintf(f, "%s\t%4.5f\n", regions[i].alias, (double)sums[run_id[i]] / (regions[i].end - regions[i].start + 1));
        by_name.erase(it);
    }
    // ... then what is left of the map, in its order, as zeros (:604-615)
    for (const auto &kv : by_name) for (uint32_t i : kv.second) fprintf(f, "%s\t%4.5f\n", regions[i].alias, 0.0);
    if (fclose(f) != 0) return fail(MSNV_EIO, "write error on %s", path);
    return MSNV_OK;
}

int coverage_write_ex(msnv_dataset &ds, int sample, const char *cov_path, const char *detail_path, const char *profile_path, const char *specific_path,
                      const msnv_cov_region *regions, uint32_t n_regions) {
    if (!ds.have_coverage) return fail(MSNV_EINVAL, "no coverage results: call msnv_coverage_run first");
    if (!ds.covx.valid) return fail(MSNV_EINVAL, "no coverage extras: call msnv_coverage_extras_run first");
    if (sample < 0 || (size_t)sample >= ds.samples.size()) return fail(MSNV_EINVAL, "sample index %d out of range", sample);
    if (specific_path && n_regions && !regions) return fail(MSNV_EINVAL, "msnv_write_coverage_ex: NULL regions");
    const size_t NC = ds.names.size();
    std::vector<unsigned long long> dense(NC * (1 + COV_BINS), 0ull);
    std::vector<int32_t> median(NC, 0);                                                  // no row: printSkipped's 0 (qaCompute.cpp:237)
    for (uint64_t r = ds.cov_row_start[(size_t)sample]; r < ds.cov_row_start[(size_t)sample + 1]; ++r) {
        memcpy(&dense[(size_t)ds.cov_row_contig[(size_t)r] * (1 + COV_BINS)], &ds.cov_acc[(size_t)r * (1 + COV_BINS)], (1 + COV_BINS) * sizeof(unsigned long long));
        median[ds.cov_row_contig[(size_t)r]] = ds.covx.row_median[(size_t)r];
    }
    if (int rc = coverage_write_rows(ds.names, ds.lengths, ds.params.cov_max, ds.samples[(size_t)sample].st, dense.data(), cov_path, detail_path, sample,
                                     ds.covx.have_median ? median.data() : nullptr)) return rc;
    if (profile_path) if (int rc = write_profile(ds, sample, profile_path)) return rc;
    if (specific_path) if (int rc = write_specific(ds, sample, specific_path, regions, n_regions)) return rc;
    return MSNV_OK;
}

// The -x file as fscanf("%s\t%d\t%d\t%s") reads it (qaCompute.cpp:344): whitespace-separated quadruples.
int coverage_regions_parse(const char *path, std::vector<std::string> &names, std::vector<int32_t> &starts, std::vector<int32_t> &ends, std::vector<std::string> &aliases) {
    FILE *f = fopen(path, "r");
    if (!f) return fail(MSNV_EIO, "Unable to open region definition file %s", path);
    std::vector<std::string> tok;
    std::string cur;
    for (int ch; (ch = fgetc(f)) != EOF;) {
        if (ch == ' ' || (ch >= '\t' && ch <= '\r')) { if (!cur.empty()) { tok.push_back(cur); cur.clear(); } }
        else cur.push_back((char)ch);
    }
    if (!cur.empty()) tok.push_back(cur);
    fclose(f);
    if (tok.size() % 4) return fail(MSNV_EDOMAIN, "region definition file %s: %zu fields, not a multiple of four (name start end alias)", path, tok.size());
    for (size_t i = 0; i < tok.size(); i += 4) {
        int32_t v[2];
        for (int j = 0; j < 2; ++j) {
            char *end = nullptr;
            const long n = strtol(tok[i + 1 + j].c_str(), &end, 10);
            if (end == tok[i + 1 + j].c_str() || *end || n < INT32_MIN || n > INT32_MAX)
                return fail(MSNV_EDOMAIN, "region definition file %s: \"%s\" is not an integer (the reference's fscanf stops making progress there)", path, tok[i + 1 + j].c_str());
            v[j] = (int32_t)n;
        }
        names.push_back(tok[i]); starts.push_back(v[0]); ends.push_back(v[1]); aliases.push_back(tok[i + 3]);
    }
    return MSNV_OK;
}

}  // namespace msnv
