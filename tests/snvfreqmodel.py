"""subpopr's snvFreqPlot (src/subpopr/R/snvFreqPlot.R:1-113) and the band of computeSnvFreqStatsThreshold (computeSnvFreqStats.R:31-46, called from
clustering.R:43-51), restated literally in numpy: every count is a comparison against cutoffsLow / cutoffsHigh in a loop over the cutoffs, as the R
has it, not the class histogram the kernel builds.  Restated from reading the R; no R was run.

A table here is positions x samples on the percent scale with NaN for a cell without coverage (-1 / NA in the file)."""
import numpy as np

CUTOFFS_LOW = [float(k) for k in range(0, 50)]              # seq(from = 0, to = 49, by = 1)
CUTOFFS_HIGH = [float(k) for k in range(100, 49, -1)]       # seq(from = 100, to = 50, by = -1): 51 entries, combos indexes the first 50
N_CUTOFFS = len(CUTOFFS_LOW)


def counts(rows, strict_lo=10.0, strict_hi=90.0):
    """low [S, 50], high [S, 50], covered [S], strict [S] as uint64: what msnv_freq_curves leaves."""
    rows = np.asarray(rows, dtype=np.float64)
    S = rows.shape[1]
    low, high = np.zeros((S, N_CUTOFFS), dtype=np.uint64), np.zeros((S, N_CUTOFFS), dtype=np.uint64)
    covered, strict = np.zeros(S, dtype=np.uint64), np.zeros(S, dtype=np.uint64)
    for s in range(S):
        freqs = rows[:, s]
        freqs = freqs[~np.isnan(freqs)]                      # freqs[freqs > -1 & !is.na(freqs)]
        covered[s] = freqs.size
        for i in range(N_CUTOFFS):
            low[s, i] = int(np.sum(freqs <= CUTOFFS_LOW[i]))
            high[s, i] = int(np.sum(freqs >= CUTOFFS_HIGH[i]))
        strict[s] = int(np.sum((freqs < strict_lo) | (freqs > strict_hi)))
    return {"low": low, "high": high, "covered": covered, "strict": strict}


def class_counts(rows):
    """The same low and high counts by the identity the kernel rests on: x <= k iff ceil(x) <= k, x >= 100 - k iff 100 - floor(x) <= k."""
    rows = np.asarray(rows, dtype=np.float64)
    S = rows.shape[1]
    low, high = np.zeros((S, N_CUTOFFS), dtype=np.uint64), np.zeros((S, N_CUTOFFS), dtype=np.uint64)
    for s in range(S):
        x = rows[:, s]
        x = x[~np.isnan(x)]
        lo_class, hi_class = np.ceil(x), 100.0 - np.floor(x)
        assert not ((lo_class < 50) & (hi_class < 50)).any()  # a cell has one class at the most
        low[s] = np.cumsum(np.bincount(lo_class[lo_class < 50].astype(np.int64), minlength=N_CUTOFFS))
        high[s] = np.cumsum(np.bincount(hi_class[hi_class < 50].astype(np.int64), minlength=N_CUTOFFS))
    return low, high


def matching_cutoff(max_prop_reads_non_homog):
    """The cutoffIndex (1..50) with cutoffIndex == maxPropReadsNonHomog * 100 + 1 in double, or 0."""
    index = float(max_prop_reads_non_homog) * 100.0 + 1.0
    for k in range(1, N_CUTOFFS + 1):
        if float(k) == index:
            return k
    return 0


def strict_band(max_prop_reads_non_homog):
    """(lo, hi) of computeSnvFreqStatsThreshold after computeClusters' fold."""
    x = float(max_prop_reads_non_homog)
    h = 1.0 - x if x > 0.5 else x
    t = h * 100.0
    return min(100.0 - t, t), max(100.0 - t, t)


def r_double(v):
    return "NaN" if v != v else "%.15g" % v


def r_logical(v):
    return "NA" if v is None else "TRUE" if v else "FALSE"


def div(a, b):
    """One double division of two integers as R does it: x / 0 is Inf, 0 / 0 NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(int(a)) / np.float64(int(b)))


def files(names, rows, species, max_prop_reads_non_homog=0.1, min_prop_homog_snv=0.8):
    """({file name: text}, result) of msnv_snvfreq_file for a table on the percent scale."""
    rows = np.asarray(rows, dtype=np.float64)
    N, S = rows.shape
    lo, hi = strict_band(max_prop_reads_non_homog)
    c = counts(rows, lo, hi)
    match = matching_cutoff(max_prop_reads_non_homog)
    cutoffs = ["cutoffIndex\tsampleID\tpropLow\tpropHigh\tpropSuffCov\tpropPass\tsampleUsedForMedoidDefn"]
    fixed = ["sampleID\tpropPass\tpropSuffCov\tsampleUsedForMedoidDefn\tpropHomogStrict\tselectedForDiscovery"]
    n_used = n_selected = n_uncovered = 0
    for s in range(S):                                       # expand.grid: cutoffIndex runs fastest
        n = int(c["covered"][s])
        n_uncovered += n == 0
        at_match = ["NA", "NA", "NA"]
        for index in range(1, N_CUTOFFS + 1):
            prop_low, prop_high, prop_cov = div(c["low"][s, index - 1], n), div(c["high"][s, index - 1], n), div(n, N)
            prop_pass = prop_low + prop_high
            used = None
            if index == match and prop_pass == prop_pass:
                used = prop_pass > min_prop_homog_snv
            cutoffs.append("\t".join([str(index), names[s], r_double(prop_low), r_double(prop_high), r_double(prop_cov), r_double(prop_pass), r_logical(used)]))
            if index == match:
                at_match = [r_double(prop_pass), r_double(prop_cov), r_logical(used)]
                n_used += bool(used)
        strict = div(c["strict"][s], n)
        selected = strict >= min_prop_homog_snv
        n_selected += selected
        fixed.append("\t".join([names[s]] + at_match + [r_double(strict), r_logical(selected)]))
    text = {species + "_snvFreq_cutoffs.tab": "\n".join(cutoffs) + "\n", species + "_snvFreq_fixed.tab": "\n".join(fixed) + "\n"}
    return text, [S, N, match, n_used, n_selected, n_uncovered, 0, 0]
