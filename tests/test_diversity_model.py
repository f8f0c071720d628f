"""The test-side model of --div / --divNS / --matched (tests/divmodel.py) against the files metaSNV_DistDiv.py wrote
(tests/golden/python_callers/diversity, made by tests/golden/make_diversity_goldens.py), and the driver's row order
against pandas' own sort_index.  No GPU: this anchors the model tests/test_gpu_diversity.py compares the device with."""
import functools
import json
import os
import random

import numpy as np
import pytest

import distmodel
import divcases
import divmodel

pd = pytest.importorskip("pandas")


def _golden(golden_dir):
    return os.path.join(golden_dir, "python_callers", "diversity")


@pytest.mark.parametrize("run", ["div_divNS", "div_matched", "divNS_matched"])
def test_model_reproduces_the_reference_files(golden_dir, run):
    g = _golden(golden_dir)
    options = json.load(open(os.path.join(g, "runs.json")))[run]["options"]
    got = divmodel.project_outputs(os.path.join(g, "proj", "filtered-m5-d2", "pop"), options)
    want_dir = os.path.join(g, "expected", run)
    assert sorted(got) == sorted(os.listdir(want_dir))
    for name, text in got.items():
        assert text == open(os.path.join(want_dir, name)).read(), (run, name)


def test_model_refuses_a_table_without_s_rows(golden_dir):
    g = _golden(golden_dir)
    assert json.load(open(os.path.join(g, "noS", "result.json")))["reference_fails"]
    with pytest.raises(ValueError):
        divmodel.project_outputs(os.path.join(g, "noS", "proj", "filtered-m5-d2", "pop"), ["--divNS"])


def test_driver_row_order_is_sort_index(tmp_path):
    """metasnv_amd.distdiv.row_order restates DataFrame.sort_index: numpy's unstable quicksort for --div (ties of > 16 rows
    are permuted), a stable order for --divNS, none when the keys are already sorted."""
    from metasnv_amd import distdiv
    rnd = random.Random(5)
    for case in range(40):
        n = rnd.choice([2, 5, 17, 40, 129, 600])
        pool = ["c%d:g:%d" % (rnd.randint(0, 2), rnd.randint(1, 30)) for _ in range(rnd.choice([1, 2, 4, 12]))]
        keys = [rnd.choice(pool) for _ in range(n)]
        if case % 5 == 0:
            keys.sort()
        path = str(tmp_path / ("t%d.freq" % case))
        with open(path, "w") as f:
            f.write("\ts0\n" + "".join("%s:A>T:%s\t0.5\n" % (k, rnd.choice("NS.")) for k in keys))
        pos = np.arange(n)
        want = pd.Series(pos, index=pd.Index(keys)).sort_index().values
        assert list(distdiv.row_order(path, stable=False)) == list(want), case
        syn = [l.split("\t")[0].split(":")[4] for l in open(path).read().splitlines()[1:]]
        s = pd.Series(pos, index=pd.MultiIndex.from_arrays([keys, syn])).sort_index()
        st = list(distdiv.row_order(path, stable=True))
        for c in "NS":                                           # within each class the rows come in the same order
            assert [r for r in s.values if syn[r] == c] == [r for r in st if syn[r] == c], case


def test_numpy_sum_is_blocked_pairwise():
    """The summation rule the kernels replay: 0.0 plus the pairwise sum of each 8192-element block."""
    def pw(a):
        n = len(a)
        if n < 8:
            r = 0.0
            for x in a:
                r += x
            return r
        if n <= 128:
            r = list(a[:8])
            i = 8
            while i < n - n % 8:
                for j in range(8):
                    r[j] += a[i + j]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            for x in a[i:]:
                res += x
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return pw(a[:n2]) + pw(a[n2:])

    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 8, 129, 8191, 8192, 8193, 17689, 30001):
        a = rng.random(n) * rng.choice([1.0, 1e12, 1e-7], n)
        t = 0.0
        for b in range(0, n, 8192):
            t = t + pw(list(a[b:b + 8192]))
        assert float(np.sum(a)) == t, n


# ---- the tables of tests/divcases.py: what they claim, numpy's tree on them, and that a wrong tree would show -------------

@functools.lru_cache(maxsize=None)
def _model_text(tmp, name, plan=None):
    """The .diversity text of one table under a plan (None: numpy's own sum), computed once per session."""
    d = os.path.join(tmp, name)
    os.makedirs(d, exist_ok=True)
    case = divcases.build(name)
    return divcases.model_outputs(case, d, plan=plan)[case.species + ".diversity"]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("divcases"))
    return lambda name, plan=None: _model_text(tmp, name, plan)


@pytest.mark.parametrize("layout", ["prefix", "suffix", "spread"])
def test_ladder_tables_hold_the_counts_they_claim(tmp_path, layout):
    name = "ladder_" + layout
    case = divcases.build(name)
    xs, sizes = divcases.parsed(name)
    names, labels, values = divmodel.read_freq(case.write(tmp_path))             # as pandas reads it
    t = divmodel.Table(divmodel.sorted_rows(labels, "div"), [":".join(l.split(":")[:3]) for l in labels], values)
    assert not t.vec and sizes == [] and np.array_equal(np.isnan(t.xs), np.isnan(xs))
    n = divcases.pair_counts(name)
    n_rows = case.meta["n_rows"]
    S = len(names)
    assert S < 30 and xs.shape == (n_rows, S) and n_rows % 64 != 0 and n_rows > 64 * 64 and n_rows <= 16500
    assert n[0][0] == n_rows
    counts = case.meta["counts"]
    assert counts == (divcases.SPREAD_COUNTS if layout == "spread" else divcases.COUNTS) and max(divcases.SPREAD_COUNTS) == 257
    ok = ~np.isnan(xs)
    for k, c in enumerate(counts, 1):
        assert n[0][k] == c and n[k][k] == c, (k, c)
        rows = np.flatnonzero(ok[:, k])
        if layout == "prefix" and c:
            assert rows[0] == 0 and rows[-1] == c - 1
        if layout == "suffix" and c:
            assert rows[0] == n_rows - c and rows[-1] == n_rows - 1 and rows[0] % 64 != 0     # it starts inside a word
        if layout == "spread" and c:
            assert len(set(rows // 64)) == c                                     # one row per word: every fill returns one element
    if layout == "suffix":
        assert sum(1 for c in counts if c and (n_rows - c) // 64 >= 1) >= 20       # leading words empty in the intersection
    if layout == "spread":
        assert len(set(np.flatnonzero(ok[:, 1 + counts.index(128)]) % 64)) > 32     # at changing lanes
    e, o = case.meta["even"], case.meta["odd"]
    assert n[e][o] == 0 and n[e][e] > 0 and n[o][o] > 0 and n[e][e] + n[o][o] == n_rows


@pytest.mark.parametrize("name", ["groups_%d" % G for G in divcases.GROUP_COUNTS] + ["groups_8193_single_8193"])
def test_group_count_tables_hold_the_counts_they_claim(name):
    case = divcases.build(name)
    xs, sizes = divcases.parsed(name)
    assert len(case.names) == 3 and len(sizes) == case.meta["G"] and sizes == case.meta["sizes"] and set(sizes) <= {2, 3}
    if len(sizes) >= 2:
        assert set(sizes) == {2, 3}
    assert xs.shape[0] == case.meta["n_single"]
    if len(sizes) >= 63:
        assert case.text.count("\t-1") > 0
    if case.meta["n_single"]:
        assert (divcases.pair_counts(name) == 8193).all() and len(sizes) == 8193


def test_group_size_table_holds_the_sizes_it_claims(tmp_path):
    case = divcases.build("group_sizes")
    xs, sizes = divcases.parsed("group_sizes")
    assert sizes == [m for m in divcases.GROUP_SIZES for _ in range(3)] and max(sizes) == divcases.MAX_TEST_GROUP
    assert divcases.GROUP_SIZES == list(range(2, 14)) + [24] and xs.shape == (6, 4)
    names, labels, values = divmodel.read_freq(case.write(tmp_path))
    keys = [":".join(l.split(":")[:3]) for l in labels]
    rows = divmodel.sorted_rows(labels, "div")
    assert rows == list(range(len(labels)))                                      # written in key order
    by_key = {}
    for r in rows:
        by_key.setdefault(keys[r], []).append(r)
    groups = [v for v in by_key.values() if len(v) > 1]
    for g, rs in enumerate(groups):
        nan = np.isnan(values[rs])
        want = [0, 1, len(rs)][g % 3]
        assert nan.sum() == want and (want == 0 or nan[:, g % 3].sum() == want), g
    # --divNS: both classes, groups in both, and groups that the class split makes smaller
    cls = divmodel.sorted_rows(labels, "divNS")
    for c in "NS":
        t = divmodel.Table(cls[c], keys, values)
        ms = sorted({(1 + int((1 + 4 * (v.shape[1] - 1)) ** .5)) // 2 for v in t.vec})
        assert t.xs.shape[0] > 0 and 24 in ms and 12 in ms and 7 in ms, (c, ms)
    # --matched: the 0.1 rule drops some keys and keeps others
    kept = set(keys[r] for r in divmodel.matched_filter(rows, keys, values))
    fate = {(len(rs), g % 3): keys[rs[0]] in kept for g, rs in enumerate(groups)}
    assert all(fate[(m, 0)] for m in divcases.GROUP_SIZES)
    assert fate[(2, 1)] and fate[(2, 2)]                                         # a length of 2 is never dropped
    assert not any(fate[(m, 1)] for m in range(3, 10)) and all(fate[(m, 1)] for m in (10, 11, 12, 13, 24))
    assert not any(fate[(m, 2)] for m in divcases.GROUP_SIZES if m > 2)
    singles = [keys[rs[0]] in kept for rs in by_key.values() if len(rs) == 1]
    assert singles.count(True) == 4 and singles.count(False) == 2


@pytest.mark.parametrize("layout", ["prefix", "suffix", "spread"])
def test_blocked_sum_is_numpys_sum_on_every_ladder_column(layout):
    """The 8192-block tree (distmodel.blocked_sum) against the installed numpy at every count of the ladder; one tree over the
    whole array is a different sum from 8193 elements on."""
    name = "ladder_" + layout
    xs, _ = divcases.parsed(name)
    flat_differs = 0
    for k in range(xs.shape[1]):
        a, b = xs[:, 0], xs[:, k]
        ok = ~(np.isnan(a) | np.isnan(b))
        a, b = a[ok], b[ok]
        p = np.ascontiguousarray(a * (1 - b) + (1 - a) * b)
        assert distmodel.blocked_sum(p[:, None])[0] == p.sum(), (k, len(p))
        assert divmodel.sequential_sum(p[:, None])[0] == functools.reduce(lambda s, x: s + x, p.tolist(), 0.0), (k, len(p))
        if len(p) <= distmodel.BLOCK:
            assert distmodel.flat_sum(p[:, None])[0] == p.sum(), (k, len(p))
        else:
            flat_differs += distmodel.flat_sum(p[:, None])[0] != p.sum()
    assert flat_differs >= 1


def _n_of(name, cell):
    return int(divcases.pair_counts(name)[cell[0]][cell[1]])


@pytest.mark.parametrize("name", ["ladder_prefix", "ladder_suffix", "ladder_spread", "groups_8193_single_8193"])
def test_one_tree_over_a_count_above_8192_prints_a_different_cell(texts, name):
    assert divcases.pair_counts(name).max() > distmodel.BLOCK
    diff = divcases.differing(texts(name, (distmodel.flat_sum, None)), texts(name))
    assert len(diff) >= 1 and all(_n_of(name, c) > distmodel.BLOCK for c in diff), diff


@pytest.mark.parametrize("name", ["ladder_prefix", "ladder_suffix", "ladder_spread"])
def test_a_plain_loop_prints_a_different_cell_within_one_leaf(texts, name):
    diff = divcases.differing(texts(name, (divmodel.sequential_sum, None)), texts(name))
    assert any(9 <= _n_of(name, c) <= 128 for c in diff), diff
    assert all(_n_of(name, c) >= 8 for c in diff), diff                          # below 8 numpy's sum is the plain loop


@pytest.mark.parametrize("name", ["groups_8193", "groups_8193_single_8193"])
def test_one_tree_over_more_than_8192_group_values_prints_a_different_cell(texts, name):
    assert divcases.build(name).meta["G"] > distmodel.BLOCK
    assert len(divcases.differing(texts(name, (None, distmodel.flat_sum)), texts(name))) >= 1
    # up to 8192 groups the two trees are the same additions
    assert divcases.differing(texts("groups_8192", (None, distmodel.flat_sum)), texts("groups_8192")) == []


def test_huge_values_reach_the_reset_of_the_kahan_sum(tmp_path):
    """1e308 six times: the sum is inf at the second, NaN at the third, and there the compensation is NaN and is reset.  The
    restated Kahan sum is pandas' own groupby().sum() on it, and the model prints an `inf` cell as to_csv does."""
    xs = [1e308] * 6
    s = c = 0.0
    reset = 0
    for x in xs:
        y = x - c
        t = s + y
        c = t - s - y
        if c != c:
            reset += 1
            c = 0.0
        s = t
    assert reset >= 1 and s != s
    got, want = divmodel.kahan(xs), divmodel.pandas_group_sum(xs)
    assert got != got and want != want
    rnd = random.Random(2)
    for _ in range(50):
        v = [rnd.choice([1e308, -1e308, 1e292, 0.1, 1 / 3, float("nan")]) for _ in range(rnd.randint(1, 12))]
        a, b = divmodel.kahan(v), divmodel.pandas_group_sum(v)
        assert a == b or (a != a and b != b), v
    case = divcases.build("huge_group")
    a = divcases.model_outputs(case, tmp_path)
    b = divcases.model_outputs(case, tmp_path, group_sum=divmodel.pandas_group_sum)
    assert a == b
    assert "\tinf" in a["huge_group.diversity"]


def test_every_seam_is_in_some_table():
    reached = set()
    for name in divcases.TABLES:
        reached |= divcases.seam_classes(name)
    assert reached == set(divcases.SEAMS)
    assert "spread fills" in divcases.seam_classes("ladder_spread") and "no single row" in divcases.seam_classes("groups_1")
