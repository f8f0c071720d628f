"""The test-side model of --dist (tests/distmodel.py) against the files metaSNV_DistDiv.py wrote (tests/golden/
python_callers/distdiv, diversity/expected/dist_matched and the long tables of dist_long, made by tests/golden/
make_dist_long_goldens.py) and against live pandas.  No GPU: this anchors the model tests/test_gpu_dist_sizes.py compares
the device with, and checks here that the swept tables tell numpy's blocked sum from a flat pairwise tree."""
import glob
import os

import numpy as np
import pytest

import distmodel
from distmodel import LONG, long_cases, long_table


@pytest.mark.parametrize("sub,out", [("distdiv/proj/filtered/pop", "distdiv/proj/distances"),
                                     ("diversity/proj/filtered-m5-d2/pop", "diversity/expected/dist_matched")])
def test_model_reproduces_the_reference_files(golden_dir, sub, out):
    tables = sorted(glob.glob(os.path.join(golden_dir, "python_callers", sub, "*.filtered.freq")))
    assert len(tables) >= 3
    for path in tables:
        names, values = distmodel.read_table(open(path).read())
        mann, allele = distmodel.dist_texts(names, values)
        stem = os.path.join(golden_dir, "python_callers", out, os.path.basename(path)[:-len(".freq")])
        assert mann == open(stem + ".mann.dist").read(), path
        assert allele == open(stem + ".allele.dist").read(), path


def test_long_cases_are_the_ones_listed(golden_dir):
    cases = long_cases(golden_dir)
    assert sorted(cases) == sorted(LONG)
    shape = {c: (cases[c]["table"]["n_pos"], cases[c]["table"]["S"]) for c in cases}
    assert shape == {"n8193x4": (8193, 4), "n20000x7": (20000, 7), "n20000x7_matched": (20000, 7), "n300000x3": (300000, 3), "n3000x70": (3000, 70)}
    assert cases["n20000x7_matched"]["options"] == ["--dist", "--matched"] and cases["n20000x7_matched"]["outdir"].endswith(".matched_pos")
    assert distmodel.n_leaves(300000) > distmodel.MAX_LEAVES_LDS


@pytest.mark.parametrize("case", LONG)
def test_model_reproduces_the_long_reference_files(golden_dir, case):
    """The blocked sum prints what the reference printed for every long table; the flat tree does not (except the table
    that fits one block).  The counts of differing cells are recorded in MEASURED.md."""
    names, text, want = long_table(golden_dir, case)
    names2, values = distmodel.read_table(text)
    assert names2 == names
    mann, allele = distmodel.dist_texts(names, values)
    assert mann == want[case + ".filtered.mann.dist"]
    assert allele == want[case + ".filtered.allele.dist"]
    flat = distmodel.dist_texts(names, values, plan=distmodel.flat_sum)
    assert flat[1] == allele                                     # a count over n_pos: no sum to get wrong
    wrong = distmodel.cells_differing(flat[0], mann)
    print(case, "cells of .mann.dist the flat plan prints differently:", wrong, "of", len(names) * (len(names) - 1) // 2)
    assert (wrong > 0) == (values.shape[0] > distmodel.BLOCK), wrong
    if case == "n3000x70":
        rows = [l.split("\t") for l in mann.splitlines()[1:]]
        assert all(rows[5][1 + j] == "" and rows[j][1 + 5] == "" for j in range(70))          # smp5 is all NaN
        assert all(l.split("\t")[1 + 5] == "0.0" for l in allele.splitlines()[1:])
        assert rows[3][1 + 9] == "0.0" and rows[9][1 + 3] == "0.0"                             # smp9 is a copy of smp3


def test_matched_case_keeps_more_than_a_block_of_rows(golden_dir):
    """The reference's --dist does not apply filt_proportion (--matched only moves the files to distances<pars>.matched_pos),
    so the distances cover all 20 000 rows; the table is still built so that more than 8192 rows would survive it."""
    import divmodel
    names, text, _ = long_table(golden_dir, "n20000x7_matched")
    _, values = distmodel.read_table(text)
    keys = ["c:-:%d" % (k + 1) for k in range(values.shape[0])]
    kept = divmodel.matched_filter(list(range(values.shape[0])), keys, values)
    assert distmodel.BLOCK < len(kept) < values.shape[0], len(kept)


def test_crossover_of_the_leaf_sums():
    """Where msnv_dist_pairs moves its leaf sums from LDS to global scratch (the comment in dist_k.hip states the same)."""
    x = distmodel.first_scratch_n_pos()
    assert x == 31 * 8192 + 7689 == 261641
    assert [distmodel.n_leaves(n) for n in (x - 1, x, 262144, 262145)] == [2048, 2049, 2048, 2049]
    assert distmodel.n_leaves(8192) == 64 and max(distmodel.n_leaves(r) for r in range(1, 8192)) == 65
    assert all(distmodel.n_leaves(n) > 2048 for n in range(262145, 262145 + 8192, 37))
    lengths = [n for _, n, _ in distmodel.sweep()]
    assert {x - 1, x, 262144, 262145} <= set(lengths)


@pytest.mark.parametrize("n_pos", [0, 1, 127, 128, 129, 8191, 8192, 8193, 16384, 16385, 3 * 8192 + 5])
def test_model_against_live_pandas(tmp_path, n_pos):
    """computeDist as the reference calls it, on lengths around the leaf and the block boundaries; also the model's
    restatement of pandas' float converter, value by value."""
    pd = pytest.importorskip("pandas")
    S = 5
    names, text = distmodel.make_table(300 + n_pos, n_pos, S, all_nan=2 if n_pos % 2 else None)
    path = str(tmp_path / "t.filtered.freq")
    open(path, "w").write(text)
    data = pd.read_table(path, index_col=0, na_values=['-1']).T
    names2, values = distmodel.read_table(text)
    assert names2 == list(data.index)
    if n_pos:
        assert np.array_equal(data.values.T.astype(np.float64), values, equal_nan=True)
    for fn, got in zip((lambda a, b: np.abs(a - b).mean(), lambda a, b: (np.abs(a - b) > .6).mean()), distmodel.dist_texts(names, values)):
        dist = pd.DataFrame([[fn(data.iloc[i], data.iloc[j]) for i in range(len(data))] for j in range(len(data))], index=data.index, columns=data.index)
        dist.to_csv(path + ".want", sep='\t')
        assert got == open(path + ".want").read()


def test_swept_tables_tell_the_blocked_sum_from_the_flat_tree():
    """The guard tests/test_gpu_dist_sizes.py asserts before it trusts a pass, checked here where the seeds were chosen."""
    guarded = [(seed, n, S) for seed, n, S in distmodel.sweep() if distmodel.must_differ(n, S)]
    assert len(guarded) == 7
    for seed, n_pos, S in guarded:
        names, text = distmodel.make_table(seed, n_pos, S)
        _, values = distmodel.read_table(text)
        blocked, flat = distmodel.dist_texts(names, values), distmodel.dist_texts(names, values, plan=distmodel.flat_sum)
        assert distmodel.cells_differing(blocked[0], flat[0]) >= 1, (seed, n_pos, S)
        assert blocked[1] == flat[1]
    for seed, n_pos, S in distmodel.sweep():                     # two whole blocks: the same tree, whatever the values
        if n_pos == 2 * distmodel.BLOCK:
            d = np.random.default_rng(seed).random((n_pos, S)) * 1e3
            assert np.array_equal(distmodel.blocked_sum(d), distmodel.flat_sum(d))
