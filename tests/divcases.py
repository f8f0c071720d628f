"""Species tables for --div / --divNS whose sizes are prescribed, not drawn: every count of valid rows, of groups and of rows
per group sits on a seam of numpy's summation tree as msnv_div_pairs (metasnv_amd/csrc/div_k.hip) replays it -- the plain
loop below 8 elements, the eight accumulators up to 128, the halving above, a fresh tree every 8192 -- or of the kernel's
staging (64 rows per fill into a ring of 256 slots).  tests/test_diversity_model.py checks without a device that the tables
hold the counts they claim and that a wrong tree would print a different cell; tests/test_gpu_div_sizes.py runs them.

Values are small-denominator fractions printed with repr (as _value of tests/test_gpu_diversity.py), NaN is `-1`.  The
coverage inputs are the same for every table: Percentage_1x 100, Average_cov 2, genome length 128, so a cell above the
diagonal is the pair's sum divided by exactly 128 and a diagonal cell by exactly 64 -- the printed repr identifies the
kernel's double.  Keys are written in ascending order (positions zero-padded), so sort_index leaves the rows where they are."""
import ctypes as C
import functools
import os
import random

import numpy as np

import divmodel

DENOMS = [1, 2, 3, 7, 40, 97, 1000, 29989, 200003]
PERC, COV, LENGTH = 100.0, 2.0, 128
BLOCK, LEAF = 8192, 128

# n of the pairs (0, k) and (k, k) of a ladder table: around 8, 16 (two rounds of the accumulators), 128 (one leaf), 136 (the
# first split that leaves two leaves with a tail), 256, the block, a block plus 8, a block plus a split leaf, two blocks
COUNTS = [0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 8191, 8192, 8193, 8199, 8200, 8201, 8321, 16384, 16385]
SPREAD_COUNTS = [c for c in COUNTS if c <= 257]
GROUP_COUNTS = [1, 2, 63, 64, 65, 128, 129, 8191, 8192, 8193]
GROUP_SIZES = list(range(2, 14)) + [24]                         # k^2 = (m(m-1)+1)^2: 8281 at m = 10, 17689 at 12, 24649 at 13, 305809 at 24
MAX_TEST_GROUP = 24                                             # no test launches a larger group
TAGS = ["N[ATG-ACG]", "S[GCT-GCC]", "."]


class Case:
    """name, species, sample names, the table's text; layout / claims as the builder states them."""

    def __init__(self, name, names, lines, **meta):
        self.name, self.species, self.names = name, name, names
        self.text = "\t" + "\t".join(names) + "\n" + "".join(lines)
        self.meta = meta

    def write(self, directory):
        path = os.path.join(str(directory), self.species + ".filtered.freq")
        with open(path, "w") as f:
            f.write(self.text)
        return path

    def coverage(self):
        return {n: PERC for n in self.names}, {n: COV for n in self.names}, LENGTH


def _value(rnd):
    c = rnd.choice(DENOMS)
    return repr(rnd.randint(0, c) / c)


def _label(species, pos, allele, tag):
    return "%s.c0:-:%07d:A>%s:%s" % (species, pos, allele, tag)


def _names(S):
    return ["s%02d.bam" % i for i in range(S)]


def _spread_row(w):
    return 64 * w + (w * 29 + 3) % 64                           # one row of word w, the lane changing from word to word


@functools.lru_cache(maxsize=None)
def ladder(layout, seed):
    """Single rows only.  Sample 0 valid everywhere, sample k valid on COUNTS[k - 1] rows, then one sample valid on the even
    64-row words only and one on the odd ones.
      prefix: the first c rows; 16421 rows (256 words and 37 rows)
      suffix: the last c rows: they start inside a word, behind words that are empty in the intersection
      spread: one row per word (SPREAD_COUNTS), the first c words for even k and the last c for odd k; 16485 rows"""
    rnd = random.Random(seed)
    counts = SPREAD_COUNTS if layout == "spread" else COUNTS
    n_rows = 16485 if layout == "spread" else 16421
    words = (n_rows + 63) // 64
    S = 1 + len(counts) + 2
    valid = np.zeros((n_rows, S), dtype=bool)
    valid[:, 0] = True
    for k, c in enumerate(counts, 1):
        if layout == "prefix":
            valid[:c, k] = True
        elif layout == "suffix":
            valid[n_rows - c:, k] = True
        else:
            for w in (range(c) if k % 2 == 0 else range(words - c, words)):
                valid[_spread_row(w), k] = True
    word_of = np.arange(n_rows) // 64
    valid[:, S - 2] = word_of % 2 == 0
    valid[:, S - 1] = word_of % 2 == 1
    name = "ladder_" + layout
    lines = []
    for r in range(n_rows):
        lines.append(_label(name, r + 1, "T", TAGS[r % 3]) + "\t" + "\t".join(_value(rnd) if ok else "-1" for ok in valid[r]) + "\n")
    return Case(name, _names(S), lines, kind="ladder", layout=layout, counts=counts, n_rows=n_rows, even=S - 2, odd=S - 1)


def _group_lines(rnd, species, pos, m, S, nan_rate=0.0, nan_row=None, nan_sample=None, tags=None):
    lines = []
    for t in range(m):
        cells = []
        for s in range(S):
            missing = rnd.random() < nan_rate or (s == nan_sample and (nan_row is None or nan_row == t))
            cells.append("-1" if missing else _value(rnd))
        lines.append(_label(species, pos, "X%d" % t, tags[t] if tags else TAGS[(pos + t) % 3]) + "\t" + "\t".join(cells) + "\n")
    return lines


@functools.lru_cache(maxsize=None)
def group_count(G, seed, n_single=0):
    """G groups of 2 rows (3 rows for every 61st), 5 % of their cells missing, 3 samples; no single row unless n_single asks for
    some, which are then valid in every sample and alternate with the groups."""
    rnd = random.Random(seed)
    name = "groups_%d" % G + ("_single_%d" % n_single if n_single else "")
    sizes = [3 if g % 61 == 1 else 2 for g in range(G)]
    lines, pos = [], 0
    for g in range(max(G, n_single)):
        if g < G:
            pos += 1
            lines += _group_lines(rnd, name, pos, sizes[g], 3, nan_rate=0.05)
        if g < n_single:
            pos += 1
            lines.append(_label(name, pos, "T", TAGS[g % 3]) + "\t" + "\t".join(_value(rnd) for _ in range(3)) + "\n")
    return Case(name, _names(3), lines, kind="group_count", G=G, sizes=sizes, n_single=n_single)


@functools.lru_cache(maxsize=None)
def group_size(seed):
    """Every size of GROUP_SIZES three times -- clean, one row missing in sample 1, every row missing in sample 2 -- between
    six single rows, 4 samples.  Classes for --divNS: the clean group all N (m even) or all S (m odd), the second alternating
    N / S row by row (its classes are groups of half the size), the third the other way round than the first.
    --matched (filt_proportion) keeps the clean groups and every pair of rows, drops a group with one missing cell below 10
    rows and keeps it from 10, drops the groups missing in a whole sample, and drops a single row with a missing cell."""
    rnd = random.Random(seed)
    name = "group_sizes"
    S = 4
    lines, pos, sizes = [], 0, []
    single_tags = ["N[ATG-ACG]", "S[GCT-GCC]", ".", "N[ATG-ACG]", "S[TA-TC]", "S[GCT-GCC]"]
    single_at = {0: 0, 7: 1, 14: 2, 21: 3, 30: 4, 38: 5}         # before which group a single row stands
    groups = [(m, v) for m in GROUP_SIZES for v in range(3)]
    for g, (m, variant) in enumerate(groups):
        if g in single_at:
            k = single_at[g]
            pos += 1
            cells = [_value(rnd) for _ in range(S)]
            if k in (2, 4):
                cells[3] = "-1"
            lines.append(_label(name, pos, "T", single_tags[k]) + "\t" + "\t".join(cells) + "\n")
        pos += 1
        first = "N[ATG-ACG]" if m % 2 == 0 else "S[GCT-GCC]"
        other = "S[GCT-GCC]" if m % 2 == 0 else "N[ATG-ACG]"
        tags = [first] * m if variant == 0 else [("N[ATG-ACG]", "S[GCT-GCC]")[t % 2] for t in range(m)] if variant == 1 else [other] * m
        lines += _group_lines(rnd, name, pos, m, S, nan_row=m // 2 if variant == 1 else None, nan_sample=(None, 1, 2)[variant], tags=tags)
        sizes.append(m)
    return Case(name, _names(S), lines, kind="group_size", G=len(groups), sizes=sizes, n_single=len(single_at))


@functools.lru_cache(maxsize=None)
def huge_group(seed):
    """One group of 3 rows whose values in sample 0 are 1e308: pandas' Kahan sum of the 6 repeated rows reaches inf at the second,
    inf - inf = NaN at the third, the compensation turns NaN and is reset; 1 - NaN closes the vector.  Against sample 1 the outer
    product overflows and the cell prints `inf`; three single rows beside it."""
    rnd = random.Random(seed)
    name = "huge_group"
    lines = [_label(name, 1, "T", TAGS[0]) + "\t" + "\t".join(_value(rnd) for _ in range(3)) + "\n"]
    for t in range(3):
        cells = ["1e308", ("0.1", "0.14285714285714285", "0.3333333333333333")[t], "-1" if t == 1 else _value(rnd)]   # sample 1: the diagonal stays finite
        lines.append(_label(name, 2, "X%d" % t, TAGS[t % 2]) + "\t" + "\t".join(cells) + "\n")
    lines += [_label(name, 3 + k, "T", TAGS[1 + k]) + "\t" + "\t".join(_value(rnd) for _ in range(3)) + "\n" for k in range(2)]
    return Case(name, _names(3), lines, kind="huge", G=1, sizes=[3], n_single=3)


@functools.lru_cache(maxsize=None)
def one_group(m, seed, S=1):
    """A table that is one group of m rows and nothing else."""
    rnd = random.Random(seed)
    name = "one_group_%d" % m
    return Case(name, _names(S), _group_lines(rnd, name, 1, m, S), kind="one_group", G=1, sizes=[m], n_single=0)


def oversized(m, seed):
    """m rows under one key, all of class S, behind one single row of each class: a table --div and --divNS both have to refuse
    when m is past the cap, --divNS only when it reaches its second class."""
    rnd = random.Random(seed)
    name = "oversized_%d" % m
    lines = [_label(name, 1 + k, "T", ("N[ATG-ACG]", "S[GCT-GCC]")[k]) + "\t" + "\t".join(_value(rnd) for _ in range(2)) + "\n" for k in range(2)]
    lines += _group_lines(rnd, name, 3, m, 2, tags=["S[GCT-GCC]"] * m)
    return Case(name, _names(2), lines, kind="oversized", G=1, sizes=[m], n_single=2)


# (builder, arguments): the seeds are chosen so that the conditions tests/test_diversity_model.py asserts hold
LADDERS = [("prefix", 11), ("suffix", 12), ("spread", 13)]
TABLES = {}
for _layout, _seed in LADDERS:
    TABLES["ladder_" + _layout] = (ladder, (_layout, _seed))
for _G in GROUP_COUNTS:
    TABLES["groups_%d" % _G] = (group_count, (_G, 100 + _G % 97))
TABLES["groups_8193_single_8193"] = (group_count, (8193, 43, 8193))
TABLES["group_sizes"] = (group_size, (41,))
TABLES["huge_group"] = (huge_group, (51,))


def build(name):
    f, args = TABLES[name]
    case = f(*args)
    assert case.name == name
    return case


@functools.lru_cache(maxsize=None)
def parsed(name):
    """(values of the single rows [rows x samples], the rows per group) as --div sees the table."""
    case = build(name)
    lines = case.text.splitlines()[1:]
    keys = [":".join(l.split("\t", 1)[0].split(":")[:3]) for l in lines]
    assert keys == sorted(keys)
    values = np.array([[np.nan if x == "-1" else float(x) for x in l.split("\t")[1:]] for l in lines], dtype=np.float64)
    single, sizes, k = [], [], 0
    while k < len(keys):
        e = k + 1
        while e < len(keys) and keys[e] == keys[k]:
            e += 1
        (single.append(k) if e - k == 1 else sizes.append(e - k))
        k = e
    return values[single].reshape(len(single), len(case.names)), sizes


@functools.lru_cache(maxsize=None)
def pair_counts(name):
    """n[i][j]: the single rows valid in both samples."""
    xs, _ = parsed(name)
    ok = (~np.isnan(xs)).astype(np.int64)
    return ok.T @ ok


SEAMS = ["empty intersection", "plain loop", "one leaf", "split tree", "multi-block tree", "spread fills", "no single row",
         "groups past a block", "outer product past one block", "past two blocks", "past three blocks"]


def seam_classes(name):
    """Which of SEAMS a --div run of the table passes through."""
    case = build(name)
    xs, sizes = parsed(name)
    n = pair_counts(name)
    ok = ~np.isnan(xs)
    out = set()
    S = len(case.names)
    for i in range(S):
        for j in range(i, S):
            c = int(n[i][j])
            if c == 0 and ok[:, i].any() and ok[:, j].any():
                out.add("empty intersection")
            if 1 <= c < 8:
                out.add("plain loop")
            if 8 <= c <= LEAF:
                out.add("one leaf")
            if LEAF < c <= BLOCK:
                out.add("split tree")
            if c > BLOCK:
                out.add("multi-block tree")
            if case.meta.get("layout") == "spread" and c > 256 and _one_per_word(ok[:, i] & ok[:, j]):
                out.add("spread fills")                         # more fills of one element than the ring has slots
    if xs.shape[0] == 0:
        out.add("no single row")
    if len(sizes) > BLOCK:
        out.add("groups past a block")
    for m in sizes:
        k2 = (m * (m - 1) + 1) ** 2
        if BLOCK < k2 <= 2 * BLOCK:
            out.add("outer product past one block")
        if 2 * BLOCK < k2 <= 3 * BLOCK:
            out.add("past two blocks")
        if k2 > 3 * BLOCK:
            out.add("past three blocks")
    return out


def _one_per_word(col):
    per_word = np.add.reduceat(col.astype(np.int64), np.arange(0, len(col), 64))
    return int(per_word.max()) == 1


def model_outputs(case, directory, mode="div", matched=False, plan=None, group_sum=divmodel.kahan):
    """{file name: text} of tests/divmodel.py for the table written into `directory`."""
    path = case.write(directory)
    h, v, L = case.coverage()
    return divmodel.species_outputs(path, mode, matched, h, v, L, plan=plan, group_sum=group_sum)


def device_outputs(ctx, case, directory, mode="div", matched=False):
    """msnv_div_file on the table written into `directory`: ({file name: text}, ms_kernel).  The row order comes from the
    function the driver uses; a refusal raises MsnvError with nothing written."""
    from metasnv_amd import _lib, distdiv
    path = case.write(directory)
    S = len(case.names)
    h, v = np.full(S, PERC), np.full(S, COV)
    order = distdiv.row_order(path, stable=mode != "div")
    names = (".diversity", ".FST") if mode == "div" else (".N_diversity", ".S_diversity")
    outs = [os.path.join(str(directory), case.species + n) for n in names]
    for o in outs:
        if os.path.exists(o):
            os.remove(o)
    P = C.POINTER
    ns, nrows, ms = C.c_int32(), C.c_uint64(), C.c_double(-1.0)
    rc = _lib.lib.msnv_div_file(ctx._h, path.encode(), _lib.DIV if mode == "div" else _lib.DIV_NS, int(matched), LENGTH,
                                h.ctypes.data_as(P(C.c_double)), v.ctypes.data_as(P(C.c_double)), S, order.ctypes.data_as(P(C.c_int64)),
                                len(order), outs[0].encode(), outs[1].encode(), C.byref(ns), C.byref(nrows), C.byref(ms))
    device_outputs.last_ms = ms.value
    _lib.check(rc)
    assert ns.value == S and nrows.value == len(order)
    return {os.path.basename(o): open(o).read() for o in outs}, ms.value


def cells(text):
    return [l.split("\t")[1:] for l in text.splitlines()[1:]]


def differing(a, b):
    """[(i, j)] with i <= j: the cells of two lower-triangular matrix texts (row j, column i) that differ."""
    ra, rb = cells(a), cells(b)
    assert len(ra) == len(rb)
    return [(i, j) for j in range(len(ra)) for i in range(j + 1) if ra[j][i] != rb[j][i]]
