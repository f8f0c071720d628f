"""Test-side model of metaSNV_DistDiv.py --dist (computeDist, metaSNV_DistDiv.py:105-124) in numpy alone: no pandas, no
device.  tests/test_dist_model.py pins it against the files the reference script wrote and against live pandas;
tests/test_gpu_dist_sizes.py compares the device with it.

  mann(i, j)   = np.abs(d1 - d2).mean() of two pandas Series: nanmean = (|a - b| with NaN replaced by 0).sum() / count of
                 the rows where neither is NaN; NaN when there is none
  allele(i, j) = (np.abs(d1 - d2) > t).mean(): NaN compares False and stays in the denominator, count / n_pos

The sum is numpy's: 0.0 plus the pairwise sum of every 8192-element block, one block after the other ("blocked").  The
"flat" plan -- one pairwise tree over the whole array, what msnv_dist_pairs built before it was corrected -- is restated
too, so that a test can require inputs on which the two differ."""
import hashlib
import json
import math
import os
import random

import numpy as np

BLOCK = 8192                                                     # numpy's reduction buffer, in elements
MAX_LEAVES_LDS = 2048                                            # dist_k.hip: leaf sums in LDS up to here, global scratch beyond
DENOMS = [1, 3, 7, 40, 97, 1000, 29989, 200003]                  # as test_distances_random_tables_against_pandas


def _leaf(a):
    """numpy's pairwise_sum on n <= 128 elements, vectorised over the columns of a [n x m]."""
    n = a.shape[0]
    if n < 8:
        res = np.zeros(a.shape[1])
        for k in range(n):
            res = res + a[k]
        return res
    n8 = n - n % 8
    r = a[:8].copy()
    for k in range(8, n8, 8):
        r += a[k:k + 8]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(n8, n):
        res = res + a[k]
    return res


def pairwise(a):
    """numpy's pairwise_sum (numpy/_core/src/umath/loops_utils.h.src) of every column of a [n x m]."""
    n = a.shape[0]
    if n <= 128:
        return _leaf(a)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:n2]) + pairwise(a[n2:])


def blocked_sum(a):
    """np.sum of every column: 0.0 + pw(block 0) + pw(block 1) + ..."""
    t = np.zeros(a.shape[1])
    for lo in range(0, a.shape[0], BLOCK):
        t = t + pairwise(a[lo:lo + BLOCK])
    return t


def flat_sum(a):
    """One pairwise tree over the whole column (equal to np.sum only up to 8192 elements)."""
    return 0.0 + (pairwise(a) if a.shape[0] else np.zeros(a.shape[1]))


def n_leaves(n, flat=False):
    """How many <= 128-element pieces the plan of an n-element sum has (what decides LDS or scratch in the kernel)."""
    def pw(n):
        if n <= 128:
            return 1
        n2 = n // 2
        n2 -= n2 % 8
        return pw(n2) + pw(n - n2)
    if flat:
        return pw(n) if n else 0
    return sum(pw(min(BLOCK, n - lo)) for lo in range(0, n, BLOCK))


def first_scratch_n_pos():
    """The shortest table whose blocked plan has more than MAX_LEAVES_LDS leaves."""
    tail = [n_leaves(r) for r in range(BLOCK + 1)]
    full = tail[BLOCK]
    best = None
    for blocks in range(MAX_LEAVES_LDS // full + 1):
        for r in range(1, BLOCK + 1):
            if blocks * full + tail[r] > MAX_LEAVES_LDS:
                n = blocks * BLOCK + r
                best = n if best is None else min(best, n)
                break
    return best


def distances(values, threshold=.6, plan=blocked_sum):
    """(mann, allele): two S x S arrays of a [n_pos x S] table (NaN = missing)."""
    n_pos, S = values.shape
    mann = np.full((S, S), math.nan)
    allele = np.full((S, S), math.nan)
    nan = np.isnan(values)
    for i in range(S):
        with np.errstate(invalid='ignore'):
            d = np.abs(values[:, i:i + 1] - values[:, i:])
        bad = nan[:, i:i + 1] | nan[:, i:]
        d[bad] = 0.0
        count = n_pos - np.count_nonzero(bad, axis=0)
        s = plan(d)
        with np.errstate(invalid='ignore', divide='ignore'):
            m = np.where(count > 0, s / count, math.nan)
            al = np.count_nonzero(d > threshold, axis=0) / np.float64(n_pos) if n_pos else np.full(S - i, math.nan)
        mann[i, i:] = m
        mann[i:, i] = m
        allele[i, i:] = al
        allele[i:, i] = al
    return mann, allele


def matrix_text(names, m):
    """DataFrame(m, index=names, columns=names).to_csv(sep='\\t'): floats as repr(), NaN as the empty string."""
    out = "\t" + "\t".join(names) + "\n" if names else '""\n'
    for i, n in enumerate(names):
        out += n + "".join("\t" + ("" if v != v else repr(float(v))) for v in m[i]) + "\n"
    return out


def dist_texts(names, values, threshold=.6, plan=blocked_sum):
    """(text of <species>.mann.dist, text of <species>.allele.dist)."""
    mann, allele = distances(values, threshold, plan)
    return matrix_text(names, mann), matrix_text(names, allele)


def cells_differing(a, b):
    """How many off-diagonal cells above the diagonal of two matrix texts differ."""
    ra, rb = [l.split("\t")[1:] for l in a.splitlines()[1:]], [l.split("\t")[1:] for l in b.splitlines()[1:]]
    assert len(ra) == len(rb)
    return sum(1 for i in range(len(ra)) for j in range(i + 1, len(ra)) if ra[i][j] != rb[i][j])


_NA = ('-1', '', 'nan', 'NaN', 'NA')
_parsed = {}
_POW10 = [float('1e%d' % k) for k in range(65)]


def parse_value(text):
    """One field as pd.read_table(na_values=['-1']) reads it: pandas' precise_xstrtod keeps at most 17 digit characters
    (a leading "0." counts one), accumulated in a double, and scales by ONE division by a power of ten -- not correctly
    rounded, and the reference's distances carry those errors (restated for plain [-]digits[.digits][e[-]digits] fields)."""
    v = _parsed.get(text)
    if v is not None:
        return v
    if text in _NA:
        v = math.nan
    else:
        t = text.lower()
        mant, _, exp = t.partition('e')
        neg = mant.startswith('-')
        whole, _, frac = mant.lstrip('+-').partition('.')
        number, digits, exponent = 0.0, 0, int(exp) if exp else 0
        for ch in whole:
            if digits < 17:
                number = number * 10.0 + float(int(ch))
                digits += 1
            else:
                exponent += 1
        for ch in frac:
            if digits >= 17:
                break
            number = number * 10.0 + float(int(ch))
            digits += 1
            exponent -= 1
        assert digits and abs(exponent) <= 64, text
        v = number * _POW10[exponent] if exponent > 0 else number / _POW10[-exponent]
        v = -v if neg else v
    _parsed[text] = v
    return v


def read_table(text):
    """(names, values [n_pos x S]) of the text of a *.filtered.freq table."""
    lines = text.splitlines()
    names = lines[0].split("\t")[1:]
    rows = [[parse_value(x) for x in l.split("\t")[1:]] for l in lines[1:] if l]
    return names, np.array(rows, dtype=np.float64).reshape(len(rows), len(names))


def make_table(seed, n_pos, S, nan_rates=None, all_nan=None, same_as=None):
    """A deterministic *.filtered.freq table: (names, text).  nan_rates: per
    sample (default .1, sample 1 NaN-heavy at .6); all_nan: a sample that is '-1' everywhere; same_as: (a, b) makes sample
    b a copy of sample a.  Values are repr(randint(0, c) / c) with mixed c, so that roundings occur."""
    rnd = random.Random(seed)
    names = ["smp%d.bam" % i for i in range(S)]
    if nan_rates is None:
        nan_rates = [0.6 if s == 1 else 0.1 for s in range(S)]
    lines = ["\t" + "\t".join(names) + "\n"]
    for k in range(n_pos):
        vals = []
        for s in range(S):
            c = rnd.choice(DENOMS)
            vals.append("-1" if (rnd.random() < nan_rates[s] or s == all_nan) else repr(rnd.randint(0, c) / c))
        if same_as:
            vals[same_as[1]] = vals[same_as[0]]
        lines.append("c:-:%d:A>T:.\t%s\n" % (k + 1, "\t".join(vals)))
    return names, "".join(lines)


PARS = "filtered-m5-d2"


def write_project(proj, species, text):
    """The least metaSNV_DistDiv.py --dist accepts: <proj>/filtered-m5-d2/pop/<species>.filtered.freq and the three files
    its file_check looks for (never read by --dist).  Returns the --filt directory."""
    pop = os.path.join(proj, PARS, "pop")
    os.makedirs(pop)
    with open(os.path.join(pop, species + ".filtered.freq"), "w") as f:
        f.write(text)
    base = os.path.basename(proj)
    for name in (base + ".all_cov.tab", base + ".all_perc.tab", "bed_header"):
        open(os.path.join(proj, name), "w").close()
    return pop


def sweep():
    """The (seed, n_pos, S) tables tests/test_gpu_dist_sizes.py runs on the device: lengths around the 128-element leaf, the
    8192-element block and the LDS / scratch crossover of the leaf sums (first_scratch_n_pos() = 261641 and 262145: scratch;
    261640 and 262144: LDS), 1 to 65 samples.  The widest and the longest are not crossed: the tables are made and parsed
    in Python."""
    x = first_scratch_n_pos()
    shapes = [(n, S) for n in (0, 1, 7, 8, 8191, 8192, 8193, 16384, 16385, 24581, 65536 + 9) for S in (1, 2, 13)]
    shapes += [(n, 65) for n in (0, 1, 8, 8193, 16385)]
    shapes += [(x - 1, 2), (x, 13), (32 * BLOCK, 2), (32 * BLOCK + 1, 2)]
    return [(7000 + k, n, S) for k, (n, S) in enumerate(shapes)]


def must_differ(n_pos, S):
    """The guard of the sweep: on a table of more than 8192 rows and at least 6 pairs the flat plan has to print at least
    one cell differently, or a kernel that still summed flat would pass.  Exactly two blocks are the one length no seed can
    separate: the flat tree splits 16384 into 8192 + 8192, so it is 0.0 + (pw(b0) + pw(b1)) = (0.0 + pw(b0)) + pw(b1), the
    blocked sum to the bit (tests/test_dist_model.py asserts that identity instead)."""
    return n_pos > BLOCK and n_pos != 2 * BLOCK and S * (S - 1) // 2 >= 6


def long_cases(golden_dir):
    return json.load(open(os.path.join(golden_dir, "python_callers", "dist_long", "cases.json")))


def long_table(golden_dir, case):
    """(names, text, {file name: text the reference wrote}) of one dist_long case, the table regenerated and its sha256 checked."""
    spec = long_cases(golden_dir)[case]
    names, text = make_table(**spec["table"])
    assert hashlib.sha256(text.encode()).hexdigest() == spec["sha256"], case
    d = os.path.join(golden_dir, "python_callers", "dist_long", case)
    return names, text, {f: open(os.path.join(d, f)).read() for f in os.listdir(d)}


LONG = ["n8193x4", "n20000x7", "n20000x7_matched", "n300000x3", "n3000x70"]
