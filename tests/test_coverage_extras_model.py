"""tests/covextmodel.py on hand-computed cases: the expected numbers and text are written out here, from qaCompute.cpp:100-123,
173-190,215,237,249-260,604-615 read by hand.  No GPU."""
import numpy as np

import covmodel
import covextmodel as xm


def _dp(*depths):
    return {t: np.array(d, dtype=np.int64) for t, d in enumerate(depths) if d is not None}


def test_window_of_five_then_four_then_a_trailing_one():
    """L = 10, W = 4: indices 0 .. 4 (five values, divisor 4), 5 .. 8, and index 9 alone under the divisor L % W = 2."""
    dp = _dp(range(1, 11))
    assert xm.window_bounds(10, 4) == [(0, 4), (5, 8), (9, 9)]
    assert xm.window_sums(dp[0], 10, 4).tolist() == [15, 30, 10]
    assert xm.profile_text(["c"], [10], dp, 4) == "c\t1\t4\t3.75000\nc\t5\t8\t7.50000\nc\t9\t10\t5.00000\n"
    assert xm.profile_text(["c"], [10], {}, 4) == "c\t1\t4\t0.00000\nc\t5\t8\t0.00000\nc\t9\t10\t0.00000\n"


def test_no_trailing_line_when_one_index_is_left():
    """L = 9, W = 4: L % W == 1, the loop's last line is at i = 8 = L - 1 and (L - 1) % W == 0."""
    dp = _dp(range(1, 10))
    assert xm.window_bounds(9, 4) == [(0, 4), (5, 8)]
    assert xm.profile_text(["c"], [9], dp, 4) == "c\t1\t4\t3.75000\nc\t5\t8\t7.50000\n"
    assert xm.profile_text(["c"], [9], {}, 4) == "c\t1\t4\t0.00000\nc\t5\t8\t0.00000\n"


def test_division_by_zero_in_the_trailing_line():
    """L = 8, W = 4: the trailing window holds indices 5 .. 7 and is divided by L % W = 0 -- " inf" for a sum that is not zero,
    "-nan" for zero on a contig with coverage, 0.00000 on one without (printSkipped prints the constant)."""
    dp = _dp([1] * 8, [1, 1, 1, 1, 1, 0, 0, 0], None)
    assert xm.window_bounds(8, 4) == [(0, 4), (5, 7)]
    want = ("c\t1\t4\t1.25000\nc\t9\t8\t inf\n"
            "d\t1\t4\t1.25000\nd\t9\t8\t-nan\n"
            "e\t1\t4\t0.00000\ne\t9\t8\t0.00000\n")
    assert xm.profile_text(["c", "d", "e"], [8, 8, 8], dp, 4) == want
    assert xm.sample_window_sums([8, 8, 8], dp, 4).tolist() == [5, 3, 5, 0, 0, 0]


def test_window_of_one_and_windows_longer_than_the_contig():
    dp = _dp([2, 3, 5, 7])
    assert xm.profile_text(["c"], [4], dp, 1) == "c\t1\t1\t5.00000\nc\t2\t2\t5.00000\nc\t3\t3\t7.00000\n"      # index 0 joins index 1; (L - 1) % 1 == 0
    assert xm.profile_text(["c"], [4], dp, 50) == "c\t1\t4\t4.25000\n"                                        # one trailing window: 17 / (4 % 50)


def test_contig_of_one_base_prints_no_profile_line():
    dp = _dp([3])
    assert xm.window_bounds(1, 4) == [] and xm.window_bounds(1, 1) == []
    assert xm.profile_text(["c"], [1], dp, 4) == "" and xm.profile_text(["c"], [1], {}, 1) == ""
    assert xm.median(dp[0]) == 3


def test_median_is_the_upper_middle_of_the_sorted_depths():
    assert xm.median([0, 5, 2, 2]) == 2           # even: sorted 0 2 2 5, index 2
    assert xm.median([4, 0, 9]) == 4              # odd: sorted 0 4 9, index 1
    assert xm.median([7, 7, 0, 0]) == 7
    assert xm.medians([4, 3, 5], _dp([0, 5, 2, 2], None, [1, 1, 1, 0, 0])).tolist() == [2, 0, 1]


def test_a_negative_last_position_sorts_last():
    """L = 2, one read of 1M at the last base: +1 at index 2 (outside), -1 at index L - 1 = 1 -- depth 0, -1.  Unsigned order puts
    the -1 behind the 0: data[1] = -1.  The window sum wraps like the reference's uint64."""
    lengths = [2]
    rec = covmodel.stream([(0, 1, "1M")])
    dp = xm.sample_depths(lengths, rec)
    assert dp[0].tolist() == [0, -1]
    assert xm.median(dp[0]) == -1
    assert xm.median([0, 0, -1]) == 0 and xm.median([5, -1]) == -1 and xm.median([5, 6, 7, -1]) == 7
    assert xm.window_sums(dp[0], 2, 4).tolist() == [(1 << 64) - 1]
    assert xm.profile_text(["c"], lengths, dp, 4) == "c\t1\t2\t9223372036854775808.00000\n"
    assert xm.region_sum(dp[0], 0, 1) == (1 << 64) - 1


def test_specific_lists_covered_contigs_first_then_the_map_in_byte_order():
    names = ["a", "b", "c"]
    dp = _dp([0, 1, 2, 3, 4], None, None)
    text = "zz 0 5 outside\nb\t1\t2\tgene_b\na\t1\t3\tgene_a1\n  a 4 4 gene_a2 Z 1 1 upper\n"
    lines = xm.parse_regions(text)
    assert lines == [("zz", 0, 5, "outside"), ("b", 1, 2, "gene_b"), ("a", 1, 3, "gene_a1"), ("a", 4, 4, "gene_a2"), ("Z", 1, 1, "upper")]
    # a has reads: its intervals in file order; then Z < b < zz (bytes), header or not, as zeros
    assert xm.specific_text(names, dp, lines) == "gene_a1\t2.00000\ngene_a2\t4.00000\nupper\t0.00000\ngene_b\t0.00000\noutside\t0.00000\n"
    assert xm.region_sums(dp, [(0, 1, 3), (0, 4, 4), (1, 1, 2)]).tolist() == [6, 4, 0]


def test_cov_text_takes_the_median_column():
    plain = "Chromosome\tSeq_lem\tAvg_Cov\nc\t4\t2.25000\nd\t3\t0.00000\n\nCov*X\tPercentage\tNr. of bases\n"
    want = "Chromosome\tSeq_len\tAvg_Cov\tMedian_Cov\nc\t4\t2.25000\t2\nd\t3\t0.00000\t0\n\nCov*X\tPercentage\tNr. of bases\n"
    assert xm.cov_text_with_median(plain, 2, [2, 0]) == want
