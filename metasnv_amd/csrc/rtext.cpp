// metasnv_amd/csrc/rtext.cpp -- what the subpopr stages (subpopr.cpp, cluster.cpp, pcoa.cpp, hclust.cpp, genotype.cpp, profile.cpp, genecorr.cpp) share on the host:
// numbers as R computes and writes them, whole files in and out, and the parsing of a field of a tab-separated table.  Declared in
// msnv_internal.h.  How a stage walks the LINES of its text stays with the stage: each follows what its reference's reader does with blank
// lines, carriage returns and the last newline.
#include <sys/stat.h>

#include <cerrno>
#include <cmath>
#include <cstring>

#include "msnv_internal.h"

namespace msnv {

// R's mean(): a long double sum over n, then the long double mean of the residuals added to it
double r_mean(const double *x, size_t n) {
    long double s = 0;
    for (size_t i = 0; i < n; ++i) s += x[i];
    s /= (long double)n;
    long double t = 0;
    for (size_t i = 0; i < n; ++i) t += x[i] - s;
    s += t / (long double)n;
    return (double)s;
}

// R's sd(): the n - 1 form, deviations from mean() summed in long double
double r_sd(const double *x, size_t n) {
    const double m = r_mean(x, n);
    long double q = 0;
    for (size_t i = 0; i < n; ++i) { const long double d = (long double)x[i] - m; q += d * d; }
    return std::sqrt((double)(q / (long double)(n - 1)));
}

void r_double(double v, std::string &out) {                            // %.15g, NaN and NA as R writes them
    if (v != v) { out += "NaN"; return; }
    char buf[40];
    snprintf(buf, sizeof buf, "%.15g", v);
    out += buf;
}

void r_value(double v, std::string &out) {                             // r_double, and Inf as R writes it
    if (std::isinf(v)) out += v > 0 ? "Inf" : "-Inf";
    else r_double(v, out);
}

int slurp(const std::string &path, std::string &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return fail(MSNV_EIO, "Cannot open %s: %s", path.c_str(), strerror(errno));
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    const bool bad = ferror(f) != 0;
    const int err = errno;
    fclose(f);
    if (bad) return fail(MSNV_EIO, "read error on %s: %s", path.c_str(), strerror(err));
    return MSNV_OK;
}

int write_text(const std::string &path, const std::string &text) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fail(MSNV_EIO, "Cannot open %s: %s", path.c_str(), strerror(errno));
    fwrite(text.data(), 1, text.size(), f);
    if (fclose(f) != 0) return fail(MSNV_EIO, "write error on %s: %s", path.c_str(), strerror(errno));
    return MSNV_OK;
}

int append_line(const std::string &path, const std::string &line) {     // write(x, file, append = T)
    FILE *f = fopen(path.c_str(), "a");
    if (!f) return fail(MSNV_EIO, "Cannot open %s: %s", path.c_str(), strerror(errno));
    fwrite(line.data(), 1, line.size(), f);
    fputc('\n', f);
    if (fclose(f) != 0) return fail(MSNV_EIO, "write error on %s: %s", path.c_str(), strerror(errno));
    return MSNV_OK;
}

int make_dir(const std::string &path) {
    if (mkdir(path.c_str(), 0777) != 0 && errno != EEXIST) return fail(MSNV_EIO, "Cannot create %s: %s", path.c_str(), strerror(errno));
    return MSNV_OK;
}

void split_span(const char *s, const char *e, char sep, std::vector<Span> &out) {
    out.clear();
    const char *b = s;
    for (const char *p = s; p <= e; ++p)
        if (p == e || *p == sep) { out.emplace_back(b, p); b = p + 1; }
}

// NA, the empty field, nan, inf and a number that overflows are refused.  strtod wants a terminator: the field is copied, onto the stack when short.
bool parse_finite(const char *s, const char *e, double &v) {
    if (s == e) return false;
    const char c = *s;
    if (!((c >= '0' && c <= '9') || c == '.' || c == '-' || c == '+')) return false;
    const size_t n = (size_t)(e - s);
    char small[64];
    std::string large;
    const char *t = small;
    if (n < sizeof small) { memcpy(small, s, n); small[n] = 0; }
    else { large.assign(s, e); t = large.c_str(); }
    char *end = nullptr;
    v = strtod(t, &end);
    return end == t + n && std::isfinite(v);
}

bool parse_small_int(const char *s, const char *e, int64_t &v) {
    const bool neg = s < e && *s == '-';
    if (s < e && (*s == '-' || *s == '+')) ++s;
    if (s == e || e - s > 9) return false;
    int64_t x = 0;
    for (; s < e; ++s) {
        if (*s < '0' || *s > '9') return false;
        x = x * 10 + (*s - '0');
    }
    v = neg ? -x : x;
    return true;
}

}  // namespace msnv
