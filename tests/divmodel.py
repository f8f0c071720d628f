"""Test-side model of metaSNV_DistDiv.py --div / --divNS / --matched (the semantics restated with numpy / pandas
primitives, one sample pair at a time).  tests/test_diversity_model.py pins it against the files the reference script
wrote (tests/golden/python_callers/diversity); tests/test_gpu_diversity.py compares the device against it on random
tables.  Slow on purpose: every sum is numpy's own.

`plan` (Table.diversity, species_outputs) replaces numpy's sum of the single rows' products and of the group values by a
restated one -- distmodel.blocked_sum (numpy's tree), distmodel.flat_sum (one tree over the whole array) or sequential_sum
below -- so that tests/test_diversity_model.py can require inputs on which a wrong tree prints a different cell.  The sums
inside a group (np.outer, np.nansum) stay numpy's.  `group_sum` replaces the Kahan restatement by pandas' own groupby."""
import math
import os

import numpy as np

NA = ('-1', '', 'nan', 'NaN', 'NA')


def read_freq(path):
    """(sample names, row labels, values [rows x samples]) as pd.read_table(path, index_col=0, na_values=['-1'])."""
    import pandas as pd
    d = pd.read_table(path, index_col=0, na_values=['-1'])
    return list(d.columns), [str(x) for x in d.index], d.values.astype(np.float64)


def sorted_rows(labels, mode):
    """Row indices in sort_index order; for --divNS a dict {'N': [...], 'S': [...]} of the rows of each class."""
    import pandas as pd
    parts = [l.split(':') for l in labels]
    keys = [p[0] + ':' + p[1] + ':' + p[2] for p in parts]
    pos = np.arange(len(labels))
    if mode == 'div':
        return list(pd.Series(pos, index=pd.Index(keys)).sort_index().values)
    syn = [p[4].split('[')[0] for p in parts]
    s = pd.Series(pos, index=pd.MultiIndex.from_arrays([keys, syn], names=['index', 'synonimity'])).sort_index()
    out = {}
    for c in ('N', 'S'):
        out[c] = [int(r) for r, cls in zip(s.values, s.index.get_level_values(1)) if cls == c]
    return out


def matched_filter(rows, keys, values):
    """filt_proportion: R rows of a key; a length (S for a unique key, R otherwise) of 2 keeps it; else drop when the NaN
    count exceeds 0.1 x that length (over the row, or over the R x S block)."""
    S = values.shape[1]
    out, k = [], 0
    while k < len(rows):
        e = k + 1
        while e < len(rows) and keys[rows[e]] == keys[rows[k]]:
            e += 1
        block = values[rows[k:e]]
        length = S if e - k == 1 else e - k
        if length == 2 or not (np.count_nonzero(np.isnan(block)) > length * 0.1):
            out.extend(rows[k:e])
        k = e
    return out


def kahan(xs):
    """pandas' groupby().sum(): Kahan-compensated, NaN skipped, compensation reset when it turns NaN."""
    s = c = 0.0
    for x in xs:
        if x == x:
            y = x - c
            t = s + y
            c = t - s - y
            if c != c:
                c = 0.0
            s = t
    return s


def pandas_group_sum(xs):
    """The same sum by pandas itself: one group through groupby().sum()."""
    import pandas as pd
    xs = np.asarray(xs, dtype=np.float64)
    return float(pd.DataFrame({'k': ['p'] * len(xs), 'x': xs}).groupby('k').sum()['x'].iloc[0])


def sequential_sum(a):
    """A plain loop over every column of a [n x m], first element first (what a kernel without numpy's tree would do)."""
    return 0.0 + (np.cumsum(np.ascontiguousarray(a.T), axis=1)[:, -1] if a.shape[0] else np.zeros(a.shape[1]))


def _sum(x, plan):
    return x.sum() if plan is None else plan(np.ascontiguousarray(x)[:, None])[0]


class Table:
    """One table's rows (in order) split into single rows and groups, with each group's k-vector per sample."""

    def __init__(self, rows, keys, values, group_sum=kahan):
        self.S = values.shape[1]
        single, groups, k = [], [], 0
        while k < len(rows):
            e = k + 1
            while e < len(rows) and keys[rows[e]] == keys[rows[k]]:
                e += 1
            (single.append(rows[k]) if e - k == 1 else groups.append(rows[k:e]))
            k = e
        self.xs = values[single]                                # [single rows x samples]
        self.vec = []                                           # per group: [samples x k]
        for g in groups:
            m = len(g)
            rep = np.tile(values[g], (m - 1, 1))                # the m rows repeated m - 1 times
            ref = np.array([1. - group_sum(rep[:, s]) for s in range(self.S)])
            self.vec.append(np.vstack([rep, ref[None, :]]).T.copy())

    def diversity(self, i, j, plan=None):
        plan_s, plan_g = plan if isinstance(plan, tuple) else (plan, plan)  # (single rows, group values)
        a, b = self.xs[:, i], self.xs[:, j]
        ok = ~(np.isnan(a) | np.isnan(b))
        a, b = a[ok], b[ok]
        nd = _sum(a * (1 - b) + (1 - a) * b, plan_s)
        if not self.vec:
            return nd
        vals = np.empty(len(self.vec))
        for g, v in enumerate(self.vec):
            out = np.outer(v[i], v[j])
            vals[g] = np.nansum(out) - np.nansum(out.diagonal())
        vals[np.isnan(vals)] = 0.0
        return _sum(vals, plan_g) + nd


def _matrix_text(names, rows):
    import io
    import pandas as pd
    buf = io.StringIO()
    pd.DataFrame(rows, index=names, columns=names).to_csv(buf, sep='\t')
    return buf.getvalue()


def species_outputs(freq_path, mode, matched, h, v, L, plan=None, group_sum=kahan):
    """{file name: text} of one species table; h / v: {sample: Percentage_1x / Average_cov}, L: genome length (int)."""
    names, labels, values = read_freq(freq_path)
    species = os.path.basename(freq_path).split('.')[0]
    S = len(names)
    parts = [l.split(':') for l in labels]
    keys = [p[0] + ':' + p[1] + ':' + p[2] for p in parts]
    hv = [np.float64(h[n]) for n in names]
    vv = [np.float64(v[n]) for n in names]
    with np.errstate(all='ignore'):
        corr = [[(min(hv[i], hv[j]) * np.int64(L)) / 100 for i in range(S)] for j in range(S)]
        for j in range(S):
            corr[j][j] = corr[j][j] / (vv[j] / (vv[j] - 1))

        def div_of(rows):
            if matched:
                rows = matched_filter(rows, keys, values)
            t = Table(rows, keys, values, group_sum)
            return [[t.diversity(i, j, plan) / corr[j][i] for i in range(j + 1)] + [math.nan] * (S - j - 1) for j in range(S)]

        if mode == 'div':
            d = div_of(sorted_rows(labels, 'div'))
            fst = [[(1 - (d[i][i] + d[j][j]) / (2 * d[j][i])) for i in range(j + 1)] + [math.nan] * (S - j - 1) for j in range(S)]
            return {species + '.diversity': _matrix_text(names, d), species + '.FST': _matrix_text(names, fst)}
        cls = sorted_rows(labels, 'divNS')
        if not cls['N'] or not cls['S']:
            raise ValueError("no N or no S rows")
        return {species + '.N_diversity': _matrix_text(names, div_of(cls['N'])), species + '.S_diversity': _matrix_text(names, div_of(cls['S']))}


def read_tab(path):
    import pandas as pd
    t = pd.read_table(path, skiprows=[1], index_col=0)
    return {str(sp): {c: float(t.loc[sp, c]) for c in t.columns} for sp in t.index}


def project_outputs(filt_dir, options):
    """{file name: text} metaSNV_DistDiv.py --div / --divNS writes for a project (the distances are not modelled)."""
    import glob
    proj = '/'.join(filt_dir.rstrip('/').split('/')[:-2])
    stem = proj + '/' + proj.split('/')[-1]
    h, v = read_tab(stem + '.all_perc.tab'), read_tab(stem + '.all_cov.tab')
    L = {}
    for line in open(proj + '/bed_header'):
        f = line.rstrip('\n').split('\t')
        L[f[0].split('.')[0]] = L.get(f[0].split('.')[0], 0) + int(f[2])
    out = {}
    for f in glob.glob(filt_dir + '/*.freq'):
        sp = os.path.basename(f).split('.')[0]
        for mode in ('div', 'divNS'):
            if '--' + mode in options:
                out.update(species_outputs(f, mode, '--matched' in options, h[sp], v[sp], L[sp]))
    return out
