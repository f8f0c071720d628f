"""msnv_div_pairs (metaSNV_DistDiv.py --div / --divNS on the device) at the sizes where its loops change shape: the tables of
tests/divcases.py, whose counts of valid rows, of groups and of rows per group are prescribed -- the plain loop, one leaf, the
split tree, a fresh tree every 8192 elements, fills of one element with the ring index wrapping inside a leaf, no single row
at all, more than 8192 groups, outer products of one group past one, two and three blocks, a Kahan sum that overflows.
Every table goes through msnv_div_file itself, and every file it writes is string-equal to the one tests/divmodel.py
(numpy and pandas; pinned without a device by tests/test_diversity_model.py, which also shows that a wrong tree would print
differently) writes.  The coverage inputs make every divisor a power of two, so a printed cell identifies the kernel's sum.
The random tables and the reference's own files are in tests/test_gpu_diversity.py."""
import os

import pytest

import divcases
import divmodel

pytestmark = pytest.mark.gpu

_reached = {}                                                   # table -> the seams its --div run passed through, once its files matched


@pytest.fixture(scope="module")
def ctx():
    from metasnv_amd import core
    c = core.Context(0)
    yield c
    c.close()


def _compare(ctx, name, directory, mode="div", matched=False, group_sum=divmodel.kahan):
    case = divcases.build(name)
    got, ms = divcases.device_outputs(ctx, case, directory, mode, matched)
    want = divcases.model_outputs(case, directory, mode, matched, group_sum=group_sum)
    assert sorted(got) == sorted(want)
    n = divcases.pair_counts(name)
    for f in sorted(want):
        wrong = divcases.differing(got[f], want[f]) if got[f].count("\n") == want[f].count("\n") else None
        print(name, mode, "matched" if matched else "all rows", f, "kernel %.3f ms," % ms, "the shape differs" if wrong is None else
              "%d cells differ (i, j, n of the single rows): %s" % (len(wrong), [(i, j, int(n[i][j])) for i, j in wrong]))
    for f in sorted(want):
        assert got[f] == want[f], (name, mode, matched, f)
    return got


def _run_table(ctx, name, directory):
    _compare(ctx, name, directory)
    _reached[name] = divcases.seam_classes(name)


@pytest.mark.parametrize("name", [n for n in divcases.TABLES if n != "huge_group"])
def test_table_matches_the_model(ctx, tmp_path, name):
    _run_table(ctx, name, tmp_path)


@pytest.mark.parametrize("mode,matched", [("divNS", False), ("div", True), ("divNS", True)])
def test_group_sizes_by_class_and_on_matched_positions(ctx, tmp_path, mode, matched):
    _compare(ctx, "group_sizes", tmp_path, mode, matched)


def test_overflowing_group_matches_pandas(ctx, tmp_path):
    """Values of 1e308: the Kahan sum of the repeated rows turns inf, then NaN, and its compensation is reset (kahan_repeated); the
    outer product against an ordinary sample overflows.  The model's group sum is pandas' groupby().sum() itself here, and the
    non-finite cells are printed as to_csv prints them."""
    got = _compare(ctx, "huge_group", tmp_path, group_sum=divmodel.pandas_group_sum)
    assert "\tinf" in got["huge_group.diversity"]
    _reached["huge_group"] = divcases.seam_classes("huge_group")


def test_every_seam_was_reached(ctx, tmp_path):
    """The counter of the sweep: every class of divcases.SEAMS was passed by a table whose files matched.  A table that this
    session has not run yet (a selection with -k) is run here."""
    for name in divcases.TABLES:
        if name not in _reached and name != "huge_group":
            _run_table(ctx, name, str(tmp_path))
    count = {s: sum(1 for v in _reached.values() if s in v) for s in divcases.SEAMS}
    print(count)
    assert all(count[s] >= 1 for s in divcases.SEAMS), count
    assert count["multi-block tree"] >= 4 and count["spread fills"] == 1 and count["no single row"] == len(divcases.GROUP_COUNTS)
    assert count["groups past a block"] == 2


def test_a_position_with_more_rows_than_the_cap_is_refused_before_any_launch(ctx, tmp_path):
    """DIV_MAX_ALLELES + 1 rows under one key: MSNV_EDOMAIN from the host, the kernel time still 0, no file written -- under
    --divNS not even the N file, though the group sits in class S.  (The cap itself is not launched here: one lane sums its
    8.8 million products for about a second per pair.)"""
    from metasnv_amd import _lib
    cap = _lib.DIV_MAX_ALLELES
    assert cap == min(max(m for m in range(2, 1000) if 8 * (m * (m - 1) + 1) ** 2 <= 2 ** 30), _lib.DIV_MAX_ALLELES_DEVICE) and cap > divcases.MAX_TEST_GROUP
    case = divcases.oversized(cap + 1, 61)
    for mode in ("div", "divNS"):
        with pytest.raises(_lib.MsnvError) as e:
            divcases.device_outputs(ctx, case, tmp_path, mode)
        assert e.value.code == _lib.EDOMAIN and "%d rows" % (cap + 1) in str(e.value) and "at most %d" % cap in str(e.value)
        assert "np.outer" in str(e.value) and "MemoryError" in str(e.value)
        assert divcases.device_outputs.last_ms == 0.0
        assert sorted(os.listdir(tmp_path)) == [case.species + ".filtered.freq"]
