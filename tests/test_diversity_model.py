"""The test-side model of --div / --divNS / --matched (tests/divmodel.py) against the files metaSNV_DistDiv.py wrote
(tests/golden/python_callers/diversity, made by tests/golden/make_diversity_goldens.py), and the driver's row order
against pandas' own sort_index.  No GPU: this anchors the model tests/test_gpu_diversity.py compares the device with."""
import json
import os
import random

import numpy as np
import pytest

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
