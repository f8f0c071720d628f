"""Test-side model of qaCompute's -m, -p W and -x FILE, in plain numpy over the per-position depth of tests/covmodel.py (marks ->
depths: the difference array of qaCompute.cpp:530-552 and its prefix sum :142-148).  tests/test_coverage_extras_model.py pins it on
hand-computed cases; tests/test_gpu_coverage_extras.py compares the library with it, exactly.

-m   data[chrSize / 2] after radix_sort (qaCompute.cpp:190,215).  radix.h sorts by unsigned bytes: a negative depth (only a contig's
     last position can hold one, from reads that hang over the end) orders behind every other.
-p W wSum = data[0]; for i = 1 .. L - 1: wSum += data[i], a line at every i % W == 0 (bounds i - W + 1, i; divisor W -- also for the
     first window, which holds W + 1 values) (:174-181); behind the loop i == L, and unless (L - 1) % W == 0 a last line with the
     bounds L - L % W + 1, L and the divisor L % W (:183-185).  wSum is a uint64: a -1 wraps.  With L % W == 0 the divisor is 0:
     x86-64 prints " inf" for a sum that is not zero and "-nan" for 0 / 0 ("%4.5f": width 4).  A contig without reads prints the
     same bounds with 0.0 (printSkipped, :249-260).
-x   per contig with reads, in header order, its intervals in file order: alias, sum(data[start .. end]) / (end - start + 1)
     (:100-123); then what is left of the std::map -- names in byte order, each with its intervals in file order -- as 0.0 (:604-615).

This build takes a contig through the no-reads path when the sample's depth is 0 everywhere on it: has
coverage = the depth is not zero somewhere, which is also when the library keeps an accumulator row."""
import numpy as np

from covmodel import marks, depths

MASK64 = (1 << 64) - 1


def sample_depths(lengths, records, min_mapq=1):
    """{tid: depth[0 .. L)} of the contigs the sample has coverage on."""
    return {t: d for t, d in depths(lengths, marks(lengths, records, min_mapq)).items() if d.any()}


# ------------------------------------------------------------------------------------------------ -m
def median(depth):
    """data[L / 2] in unsigned order (qaCompute.cpp:190,215)."""
    d = np.asarray(depth, dtype=np.int64)
    order = np.concatenate([np.sort(d[d >= 0]), np.sort(d[d < 0])])
    return int(order[len(d) // 2])


def medians(lengths, dp):
    """[contig] int32; 0 for a contig without coverage (:237)."""
    return np.array([median(dp[t]) if t in dp else 0 for t in range(len(lengths))], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ -p W
def window_bounds(L, W):
    """[(first index, last index)] of the windows of a contig: window 0 starts at index 0, window k >= 1 at k W + 1; full windows end
    at (k + 1) W <= L - 1, the trailing one (if (L - 1) % W != 0) at L - 1.  None for L == 1."""
    if L < 2:
        return []
    full = (L - 1) // W
    out = [(0 if k == 0 else k * W + 1, (k + 1) * W) for k in range(full)]
    if (L - 1) % W != 0:
        out.append((0 if full == 0 else full * W + 1, L - 1))
    return out


def window_sums(depth, L, W):
    """uint64 sums (mod 2^64) of the windows of one contig; depth None = no coverage."""
    b = window_bounds(L, W)
    if depth is None or not b:
        return np.zeros(len(b), dtype=np.uint64)
    pre = np.concatenate([[0], np.cumsum(np.asarray(depth, dtype=np.int64))])          # (|sum| < 2^63 for any depth the tests reach)
    lo, hi = np.array(b, dtype=np.int64).T
    return (pre[hi + 1] - pre[lo]).astype(np.uint64)                                   # a negative sum wraps


def sample_window_sums(lengths, dp, W):
    """One sample's sums, contig-major in header order."""
    parts = [window_sums(dp.get(t), int(L), W) for t, L in enumerate(lengths)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def profile_text(names, lengths, dp, W):
    out = []
    for t, (name, L) in enumerate(zip(names, lengths)):
        L = int(L)
        if L < 2:
            continue
        sums = window_sums(dp[t], L, W) if t in dp else None
        full = (L - 1) // W
        for k in range(full):                                                            # :179 / :255
            out.append("%s\t%d\t%d\t%4.5f\n" % (name, k * W + 1, (k + 1) * W, float(int(sums[k])) / W if sums is not None else 0.0))
        if (L - 1) % W != 0:                                                             # :183-185 / :258-260
            rest = L % W
            if sums is None:
                val = "%4.5f" % 0.0
            elif rest == 0:
                val = " inf" if int(sums[full]) else "-nan"
            else:
                val = "%4.5f" % (float(int(sums[full])) / rest)
            out.append("%s\t%d\t%d\t%s\n" % (name, L - rest + 1, L, val))
    return "".join(out)


# ------------------------------------------------------------------------------------------------ -x FILE
def parse_regions(text):
    """fscanf("%s\\t%d\\t%d\\t%s") (:344): whitespace-separated quadruples -> [(name, start, end, alias)]."""
    tok = text.split()
    assert len(tok) % 4 == 0
    return [(tok[i], int(tok[i + 1]), int(tok[i + 2]), tok[i + 3]) for i in range(0, len(tok), 4)]


def region_sum(depth, start, end):
    """sum(data[start .. end]) as the uint64 covSum of :107-116; depth None = no coverage."""
    if depth is None:
        return 0
    assert 0 <= start <= end < len(depth)
    return int(np.asarray(depth[start:end + 1], dtype=np.int64).sum()) & MASK64


def region_sums(dp, regions):
    """[region] uint64 for (tid, start, end) triples."""
    return np.array([region_sum(dp.get(t), s, e) for t, s, e in regions], dtype=np.uint64)


def specific_text(names, dp, lines):
    """lines: [(contig name, start, end, alias)] of the -x file."""
    by_name = {}
    for ln in lines:
        by_name.setdefault(ln[0], []).append(ln)
    out = []
    for t, name in enumerate(names):                                                     # contigs with reads, header order (:100-123)
        if t in dp and name in by_name:
            for (_, s, e, alias) in by_name.pop(name):
                out.append("%s\t%4.5f\n" % (alias, float(region_sum(dp[t], s, e)) / (e - s + 1)))
    for name in sorted(by_name, key=lambda n: n.encode()):                               # the rest of the map (:604-615)
        for (_, _, _, alias) in by_name[name]:
            out.append("%s\t%4.5f\n" % (alias, 0.0))
    return "".join(out)


# ------------------------------------------------------------------------------------------------ OUT with -m
def cov_text_with_median(plain_text, n_contigs, med):
    """The OUT of `-m` from the OUT without it: the header spells Seq_len and takes Median_Cov (:437), every contig row the median
    (:215,237); the rest of the file is the same."""
    lines = plain_text.split("\n")
    assert lines[0] == "Chromosome\tSeq_lem\tAvg_Cov"
    lines[0] = "Chromosome\tSeq_len\tAvg_Cov\tMedian_Cov"
    for c in range(n_contigs):
        lines[1 + c] += "\t%d" % int(med[c])
    return "\n".join(lines)
