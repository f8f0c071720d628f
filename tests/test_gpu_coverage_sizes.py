"""msnv_coverage_tiles at the sizes where its forms change, against the integer model of tests/covmodel.py -- word for word.

The kernel takes one interval per lane up to 64 intervals of a (tile, sample) pair, four per lane up to 256 and steps of 256 beyond; it
keeps 16-bit biased half-words up to 32 767 intervals and one word per position above; it packs the histogram into byte fields, then
16-bit fields; it loads up to three entries behind a pair's last interval, carries LDS from one pair of a work item to the next and
spreads tiles over cov_copies accumulator copies.  The text of .cov / .cov.detail shows neither hist[0] nor a covSum that is off by
less than the fifth decimal of covSum / L, so every case compares Dataset.coverage_accumulators() -- all 17 words of every (sample,
contig) -- with np.array_equal, and reads the fetched cov_pairs / cov_work tables to see that the pair it was built for holds the
intended number of intervals and shares a work item with the intended neighbours.  The record sets are hand-placed
(covmodel.group_a .. group_f, built once per process); tests/test_coverage_model.py pins the model against the oracle on each.

Every case runs under the default knobs and under MSNV_COV_NARROW_MAX=1 (every item through the one-word-per-position variant);
groups d and e also with MSNV_COV_ITEM=1 and =300 (other cuts of the work items)."""
import numpy as np
import pytest

import covmodel
import orc
from metasnv_amd import core

pytestmark = pytest.mark.gpu

VARIANTS = {"default": {}, "wide": {"MSNV_COV_NARROW_MAX": "1"}, "item1": {"MSNV_COV_ITEM": "1"}, "item300": {"MSNV_COV_ITEM": "300"}}
RUNS = [(n, v) for n in covmodel.CASE_NAMES for v in ("default", "wide")] + [(n, v) for n in covmodel.CASE_NAMES if n[0] in "de" for v in ("item1", "item300")]


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def _index(ds):
    """({sample: [intervals of its pairs, tiles ascending]}, {tile: [[samples of a work item], ...]}, work items of the wide variant) from the
    fetched tables (TilePair: sample, lo, hi, row, ...; WorkItem: tile, pair_lo, pair_hi); every pair belongs to exactly one work item."""
    pairs = ds.column("cov_pairs").view(np.uint32).reshape(-1, 8)
    work = ds.column("cov_work").view(np.uint32).reshape(-1, 16)
    seen = np.zeros(len(pairs), dtype=np.int32)
    by_sample, items = {}, {}
    for w in work:
        t, lo, hi = int(w[0]), int(w[1]), int(w[2])
        assert 0 < hi - lo <= 4, (t, lo, hi)
        seen[lo:hi] += 1
        items.setdefault(t, []).append((lo, [int(pairs[k, 0]) for k in range(lo, hi)]))
        for k in range(lo, hi):
            by_sample.setdefault(int(pairs[k, 0]), []).append((t, int(pairs[k, 2]) - int(pairs[k, 1])))
    assert (seen == 1).all(), "pairs outside every work item or in two"
    return ({s: sorted(v) for s, v in by_sample.items()}, {t: [x[1] for x in sorted(v)] for t, v in items.items()})


def _check_index(case, variant, ds, sizes):
    """The device's pairs hold the model's interval counts -- every pair, the ones the case was built for among them -- and the work
    items group the samples as intended."""
    by_sample, items = _index(ds)
    tile_of = {}
    for s in range(len(case.samples)):
        want = sorted((t, k, n) for (ss, t, k), n in sizes.items() if ss == s)
        got = by_sample.get(s, [])
        assert [n for (_, n) in got] == [n for (_, _, n) in want], (case.name, s, "intervals per pair")
        for (gt, _), (t, k, _) in zip(got, want):
            assert tile_of.setdefault((t, k), gt) == gt
    for key, n in case.pairs.items():
        assert sizes[key] == n, (case.name, key)
    if variant in ("default", "wide"):
        for key, groups in case.items.items():
            assert items[tile_of[key]] == groups, (case.name, key, items[tile_of[key]])
    if variant == "item1":
        assert all(len(g) == 1 for v in items.values() for g in v)


def _accumulators(case, ds, acc_model):
    acc = ds.coverage_accumulators()
    assert acc.dtype == np.uint64 and acc.shape == acc_model.shape
    if not np.array_equal(acc, acc_model):
        s, c, w = [int(x[0]) for x in np.nonzero(acc != acc_model)]
        raise AssertionError("%s: sample %d contig %d word %d (0 = covSum, 1 + b = bin b): %d, the model has %d\n%s\n%s"
                             % (case.name, s, c, w, acc[s, c, w], acc_model[s, c, w], acc[s, c], acc_model[s, c]))
    for s in range(len(case.samples)):
        for c, L in enumerate(case.lengths):
            if case.depth_never_negative(s, c):
                assert int(acc[s, c, 1:].sum()) == L, (case.name, s, c)
    return acc


@pytest.mark.parametrize("name,variant", RUNS)
def test_accumulators_equal_the_model(name, variant, ctx, tmp_path, monkeypatch):
    case = covmodel.cases()[name]
    acc_model, sizes = case.model()
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    params = core.default_params(cov_max=case.cov_max)
    ds = core.Dataset(ctx, case.names, case.lengths, case.seqs, params)
    try:
        for s in case.samples:
            ds.add_sample_records(s)
        ds.finalize()
        _check_index(case, variant, ds, sizes)
        ds.coverage_run()
        acc = _accumulators(case, ds, acc_model)
        if case.seqs is not None:                              # the same index under the fused run
            ds.fused_run()
            assert np.array_equal(ds.coverage_accumulators(), acc)
            _accumulators(case, ds, acc_model)
        if variant == "default":                               # the text, against the oracle
            checked = 0
            for i, s in enumerate(case.samples):
                try:
                    want = orc.qacompute(case.names, case.lengths, s, max_cov=params.cov_max, min_mapq=params.cov_min_mapq)
                except orc.OrcError:
                    continue                                   # (a sample without mapped reads: undefined in the reference)
                cp, dp = str(tmp_path / "x.cov"), str(tmp_path / "x.cov.detail")
                ds.write_coverage(i, cp, dp)
                assert (open(cp).read(), open(dp).read()) == want, (name, i)
                checked += 1
            assert checked > 0
    finally:
        ds.close()
