"""The test-side model of qaCompute's arithmetic (tests/covmodel.py) against the oracle's text (oracle/orc_qacompute.c) on every record
set of tests/test_gpu_coverage_sizes.py and on the record sets of the CIGAR-quirk and contig-end tests of tests/test_gpu_parity.py, at
cov_max 1, 10 and 15: every .cov.detail row, every Avg_Cov field as printed and the base counts of the Cov*X block.  No GPU: this is
what entitles the GPU tests to trust the model for hist[0] and the exact covSum, which the text does not show."""
import numpy as np
import pytest

import bamtools as bt
import covmodel
import orc


def _against_oracle(names, lengths, samples, acc_of, min_mapq=1):
    checked = 0
    for max_cov in (1, 10, 15):
        acc = acc_of(max_cov)
        for i, s in enumerate(samples):
            try:
                cov, detail = orc.qacompute(names, lengths, s, max_cov=max_cov, min_mapq=min_mapq)
            except orc.OrcError:
                assert not any(not (r["flag"] & 4) and r["tid"] >= 0 for r in bt.iter_records(s))      # no mapped read: undefined in the reference
                assert not acc[i].any()
                continue
            assert covmodel.detail_text(names, lengths, acc[i], max_cov) == detail, (i, max_cov)
            rows, counts = covmodel.parse_cov_text(cov, len(names), max_cov)
            assert covmodel.avg_rows(names, lengths, acc[i]) == rows, (i, max_cov)
            assert covmodel.covx_counts(acc[i], max_cov) == counts, (i, max_cov)
            assert not acc[i][:, 2 + max_cov:].any()
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", covmodel.CASE_NAMES)
def test_model_prints_what_the_oracle_prints(name):
    case = covmodel.cases()[name]
    _against_oracle(case.names, case.lengths, case.samples, lambda m: case.model(m)[0])
    acc, sizes = case.model()
    for key, n in case.pairs.items():                        # the record set holds the pairs it was built for
        assert sizes.get(key) == n, (key, sizes.get(key), n)
    for s in range(len(case.samples)):
        for c, L in enumerate(case.lengths):
            if case.depth_never_negative(s, c):
                assert int(acc[s, c, 1:].sum()) == L


def test_group_a_reaches_every_bin():
    acc, _ = covmodel.cases()["a_last769"].model(15)
    assert (acc[:, 0, 1:].sum(axis=0) > 0).all()


def _plain(names, lengths, samples, min_mapq=1):
    def acc_of(max_cov):
        return np.stack([covmodel.accumulators(lengths, covmodel.depths(lengths, covmodel.marks(lengths, s, min_mapq)), max_cov) for s in samples])
    _against_oracle(names, lengths, samples, acc_of, min_mapq)
    return acc_of


def test_model_on_the_cigar_quirks_and_filters():
    """The record set of test_gpu_parity.py::test_coverage_cigar_quirks_and_filters, also with cov_min_mapq 0."""
    L = 300
    ref = "ACGT" * 75
    rec = [
        bt.make_record(0, 10, "5S20M", "N" * 5 + ref[10:30]),
        bt.make_record(0, 10, "10M5I10M", ref[10:20] + "GGGGG" + ref[20:30]),
        bt.make_record(0, 12, "10M4D10M", ref[12:22] + ref[26:36]),
        bt.make_record(0, 15, "8=4X8=", ref[15:35]),
        bt.make_record(0, 20, "10M3S", ref[20:30] + "NNN"),
        bt.make_record(0, 30, "20M", ref[30:50], mapq=0),
        bt.make_record(0, 30, "20M", ref[30:50], flag=0x400),
        bt.make_record(0, 30, "20M", ref[30:50], flag=0x100 | 0x200 | 0x1),
        bt.make_record(0, 280, "19M", ref[280:299]),
        bt.make_record(0, 285, "14M", ref[285:299]),
        bt.make_record(-1, -1, "*", "ACGT", flag=4),
    ]
    s1 = bt.records(*rec)
    s2 = bt.records(*[bt.make_record(1, 5 * k, "50M", "A" * 50, name="k%d" % k) for k in range(60)])
    for min_mapq in (1, 0):
        _plain(["c1", "c2"], [L, 400], [s1, s2], min_mapq)


def test_model_on_reads_at_the_contig_end():
    """The record set of test_gpu_parity.py::test_coverage_reads_at_the_contig_end_do_not_fail_the_run: the last index at depth -2 lands in
    no bin and enters the sum."""
    L = 100
    ref = "ACGT" * 25
    s = bt.records(*[bt.make_record(0, 60, "40M", ref[60:100], name="c%d" % i) for i in range(3)],
                   bt.make_record(0, 90, "5M8I2M", ref[90:95] + "G" * 8 + "AC", name="t2"),
                   bt.make_record(0, 97, "2M", "CG", name="t0"),
                   bt.make_record(0, 99, "1M4S", "ACGTA", name="t1"))
    acc = _plain(["c1", "c2"], [L, 50], [s])(10)
    assert int(acc[0, 0, 1:].sum()) == L - 1 and not acc[0, 1].any()
