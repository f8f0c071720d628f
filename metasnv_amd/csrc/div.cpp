// metasnv_amd/csrc/div.cpp -- host side of metaSNV_DistDiv.py --div / --divNS (computeDiv / computeDivNS,
// metaSNV_DistDiv.py:182-301): read one `<species>.filtered.freq` table with its row labels, key the rows by
// contig:gene:pos (and N / S for --divNS), apply the caller's sort order and the --matched filter (filt_proportion),
// split the rows into single rows and multi-allelic groups, run the pair kernel (div_k.hip), then divide by the
// coverage corrections and write the lower-triangular matrices the way DataFrame.to_csv(sep='\t') does.
#include <cmath>
#include <cstring>

#include "dataset.h"
#include "device.h"

namespace msnv {

namespace {

// filt_proportion (metaSNV_DistDiv.py:199-204) for one key of R rows: True = drop.  data.loc[key] is the row (a Series of
// S values) when the key is unique, the R x S frame otherwise; a length of 2 empties it (iloc[1:1]).
bool drop_key(const std::vector<double> &rows, size_t S, const std::vector<uint64_t> &sel, size_t lo, size_t hi) {
    const size_t R = hi - lo;
    const size_t len = R == 1 ? S : R;
    if (len == 2) return false;
    long nans = 0;
    for (size_t k = lo; k < hi; ++k)
        for (size_t s = 0; s < S; ++s) { const double v = rows[sel[k] * S + s]; nans += v != v; }
    return (double)nans > (double)len * 0.1;
}

// One table's rows ready for the pair kernel: the single rows and the multi-allelic groups as sample-major columns (div_k.hip)
struct PairTable {
    std::vector<double> xs, xg;
    std::vector<uint64_t> bits;                                 // bit r % 64 of word r / 64: single row r present
    std::vector<long> goff{0};
    long ns = 0, nw = 0, ng = 0;
};

// The host half of compute_diversity for one table, given its rows in order (indices into `rows`): the --matched filter, the split into
// single rows and groups, the refusal of a group no launch should be given.  Nothing here touches the device.
int pair_table(const std::vector<double> &rows, size_t S, const std::vector<std::string> &keys, std::vector<uint64_t> sel, bool matched, PairTable &t) {
    if (matched) {
        std::vector<uint64_t> kept;
        for (size_t lo = 0; lo < sel.size();) {
            size_t hi = lo + 1;
            while (hi < sel.size() && keys[sel[hi]] == keys[sel[lo]]) ++hi;
            if (!drop_key(rows, S, sel, lo, hi)) kept.insert(kept.end(), sel.begin() + lo, sel.begin() + hi);
            lo = hi;
        }
        sel.swap(kept);
    }
    std::vector<uint64_t> single, grouped;
    for (size_t lo = 0; lo < sel.size();) {
        size_t hi = lo + 1;
        while (hi < sel.size() && keys[sel[hi]] == keys[sel[lo]]) ++hi;
        if (hi - lo == 1) single.push_back(sel[lo]);
        else {
            if (hi - lo > DIV_MAX_ALLELES) {
                const double k = (double)(hi - lo) * (double)(hi - lo - 1) + 1;
                return fail(MSNV_EDOMAIN, "position %s has %zu rows, at most %u are computed: the reference's np.outer of the %.0f values per sample allocates "
                                          "%.1f GiB there (MemoryError where it cannot)", keys[sel[lo]].c_str(), hi - lo, DIV_MAX_ALLELES, k, 8.0 * k * k / 1073741824.0);
            }
            grouped.insert(grouped.end(), sel.begin() + lo, sel.begin() + hi);
            t.goff.push_back((long)grouped.size());
        }
        lo = hi;
    }
    const long ns = t.ns = (long)single.size(), nw = t.nw = (ns + 63) / 64, ng = t.ng = (long)grouped.size();
    t.xs.resize(S * ns);                                        // sample-major columns
    t.xg.resize(S * ng);
    t.bits.assign(S * nw, 0);
    for (long r = 0; r < ns; ++r)
        for (size_t s = 0; s < S; ++s) {
            const double v = rows[single[r] * S + s];
            t.xs[s * ns + r] = v;
            if (v == v) t.bits[s * nw + r / 64] |= 1ull << (r % 64);
        }
    for (long r = 0; r < ng; ++r)
        for (size_t s = 0; s < S; ++s) t.xg[s * ng + r] = rows[grouped[r] * S + s];
    return MSNV_OK;
}

// compute_diversity for every pair (i <= j) of one prepared table
int diversity_pairs(msnv_ctx *ctx, const PairTable &t, size_t S, std::vector<double> &cd, double *ms_kernel) {
    cd.assign(S * S, std::nan(""));
    if (!S) return MSNV_OK;
    return dev_div(t.xs.data(), t.bits.data(), t.ns, t.nw, t.xg.data(), t.goff.data(), (long)t.goff.size() - 1, t.ng, (int)S, ctx->stream, cd.data(), ms_kernel);
}

}  // namespace

int div_file(msnv_ctx *ctx, const char *freq_path, int32_t mode, int32_t matched, int64_t genome_length, const double *h, const double *v,
             int32_t n_cov, const int64_t *row_order, uint64_t n_order, const char *out_a, const char *out_b, int32_t *n_samples_out,
             uint64_t *n_rows_out, double *ms_kernel) {
    std::vector<std::string> names, labels;
    std::vector<double> rows;
    uint64_t n_rows = 0;
    if (int rc = read_freq(freq_path, names, &labels, rows, n_rows)) return rc;
    const size_t S = names.size();
    if ((size_t)n_cov != S) return fail(MSNV_EINVAL, "%s: %zu samples, %d coverage values given", freq_path, S, n_cov);
    if (n_order != n_rows) return fail(MSNV_EINVAL, "%s: %llu rows, a row order of %llu given", freq_path, (unsigned long long)n_rows, (unsigned long long)n_order);
    // the row keys: contig:gene:pos, and the synonymity (field 4 up to '[') for --divNS
    std::vector<std::string> keys(n_rows), syn(mode == 1 ? n_rows : 0);
    for (uint64_t r = 0; r < n_rows; ++r) {
        const std::string &l = labels[r];
        size_t c[4], at = 0;
        int nf = 0;
        for (; nf < 4; ++nf) { const size_t p = l.find(':', at); if (p == std::string::npos) break; c[nf] = p; at = p + 1; }
        if (nf < 2 || (mode == 1 && nf < 4)) return fail(MSNV_EFORMAT, "%s: row '%s' has fewer than %d ':'-separated fields", freq_path, l.c_str(), mode == 1 ? 5 : 3);
        keys[r] = l.substr(0, nf >= 3 ? c[2] : l.size());
        if (mode == 1) {
            const size_t e = l.find(':', c[3] + 1);
            const std::string f4 = l.substr(c[3] + 1, e == std::string::npos ? std::string::npos : e - c[3] - 1);
            syn[r] = f4.substr(0, f4.find('['));
        }
    }
    // the caller's order (numpy's argsort of the keys, as sort_index does it): a permutation that sorts the keys
    std::vector<uint64_t> order(n_rows);
    std::vector<char> seen(n_rows, 0);
    for (uint64_t k = 0; k < n_rows; ++k) {
        const int64_t r = row_order[k];
        if (r < 0 || (uint64_t)r >= n_rows || seen[r]) return fail(MSNV_EINVAL, "%s: the row order is not a permutation of the %llu rows", freq_path, (unsigned long long)n_rows);
        seen[r] = 1;
        order[k] = (uint64_t)r;
        if (k && keys[order[k - 1]] > keys[r]) return fail(MSNV_EINVAL, "%s: the row order does not sort the keys ('%s' after '%s')", freq_path, keys[r].c_str(), keys[order[k - 1]].c_str());
    }
    if (ms_kernel) *ms_kernel = 0;
    // the coverage corrections (metaSNV_DistDiv.py:207-220): corr[j][i] = (min(h_i, h_j) * L) / 100, the diagonal divided by v / (v - 1)
    const double L = (double)genome_length;
    std::vector<double> corr(S * S);
    for (size_t j = 0; j < S; ++j)
        for (size_t i = 0; i < S; ++i) corr[j * S + i] = ((h[j] < h[i] ? h[j] : h[i]) * L) / 100;
    for (size_t j = 0; j < S; ++j) corr[j * S + j] = corr[j * S + j] / (v[j] / (v[j] - 1));
    auto divide = [&](const std::vector<double> &cd) {          // div[j][i] for i <= j, NaN above (printed empty)
        std::vector<double> d(S * S, std::nan(""));
        for (size_t j = 0; j < S; ++j)
            for (size_t i = 0; i <= j; ++i) d[j * S + i] = cd[i * S + j] / corr[j * S + i];
        return d;
    };
    std::vector<double> cd;
    if (mode == 0) {
        PairTable t;
        if (int rc = pair_table(rows, S, keys, order, matched != 0, t)) return rc;
        if (int rc = diversity_pairs(ctx, t, S, cd, ms_kernel)) return rc;
        const std::vector<double> d = divide(cd);
        std::vector<double> fst(S * S, std::nan(""));
        for (size_t j = 0; j < S; ++j)
            for (size_t i = 0; i <= j; ++i) fst[j * S + i] = 1 - (d[i * S + i] + d[j * S + j]) / (2 * d[j * S + i]);
        if (int rc = write_matrix(out_a, names, d)) return rc;
        if (int rc = write_matrix(out_b, names, fst)) return rc;
    } else {
        std::vector<uint64_t> sel[2];
        for (uint64_t r : order) {
            if (syn[r] == "N") sel[0].push_back(r);
            else if (syn[r] == "S") sel[1].push_back(r);
        }
        if (sel[0].empty() || sel[1].empty())                   // metaSNV_DistDiv.py:252-260
            return fail(MSNV_EDOMAIN, "%s: no %s SNV in the table: synonymous and non-synonymous diversity need both types (was the SNV calling "
                                      "given gene annotation?)", freq_path, sel[0].empty() ? "non-synonymous (N)" : "synonymous (S)");
        PairTable t[2];                                         // both classes are prepared before either is launched: a refusal leaves no file
        for (int c = 0; c < 2; ++c)
            if (int rc = pair_table(rows, S, keys, sel[c], matched != 0, t[c])) return rc;
        for (int c = 0; c < 2; ++c) {
            if (int rc = diversity_pairs(ctx, t[c], S, cd, ms_kernel)) return rc;
            if (int rc = write_matrix(c == 0 ? out_a : out_b, names, divide(cd))) return rc;
        }
    }
    if (n_samples_out) *n_samples_out = (int32_t)S;
    if (n_rows_out) *n_rows_out = n_rows;
    return MSNV_OK;
}

}  // namespace msnv
