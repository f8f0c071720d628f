"""tests/snvfreqmodel.py, the literal restatement of subpopr's snvFreqPlot, held to a table worked by hand, and the identity the device kernel
(csrc/snvfreq_k.hip) rests on held to the literal comparisons.  No GPU."""
import numpy as np
import pytest

import snvfreqcases as cases
import snvfreqmodel as model

NA = float("nan")
HAND = np.array([[0.0, 100.0, NA],
                 [5.0, 90.0, NA],
                 [10.0, 50.0, NA],
                 [49.0, 49.5, NA],
                 [95.0, 51.0, NA],
                 [NA, 0.5, NA]])


def test_hand_worked_table():
    c = model.counts(HAND, 10.0, 90.0)
    # column 0 holds 0, 5, 10, 49, 95: <= k takes 0 from k = 0, 5 from 5, 10 from 10, 49 at 49; >= 100 - k takes 95 from k = 5
    assert c["low"][0].tolist() == [1] * 5 + [2] * 5 + [3] * 39 + [4]
    assert c["high"][0].tolist() == [0] * 5 + [1] * 45
    # column 1 holds 100, 90, 50, 49.5, 51, 0.5: 0.5 is <= k from k = 1, 49.5 and 50 never; 100 from k = 0, 90 from 10, 51 at 49 (cutoff 51)
    assert c["low"][1].tolist() == [0] + [1] * 49
    assert c["high"][1].tolist() == [1] * 10 + [2] * 39 + [3]
    assert c["low"][2].tolist() == [0] * 50 and c["high"][2].tolist() == [0] * 50
    assert c["covered"].tolist() == [5, 6, 0]
    assert c["strict"].tolist() == [3, 2, 0]                 # < 10 | > 90: {0, 5, 95} (10 is not < 10), {100, 0.5} (90 is not > 90)
    low, high = model.class_counts(HAND)
    assert (low == c["low"]).all() and (high == c["high"]).all()


def test_hand_worked_files():
    text, result = model.files(["A", "B", "C"], HAND, "sp")
    rows = text["sp_snvFreq_cutoffs.tab"].split("\n")
    assert rows[0] == "cutoffIndex\tsampleID\tpropLow\tpropHigh\tpropSuffCov\tpropPass\tsampleUsedForMedoidDefn"
    assert len(rows) == 1 + 150 + 1 and rows[-1] == ""
    assert [r.split("\t")[:2] for r in rows[1:151]] == [[str(k), nm] for nm in "ABC" for k in range(1, 51)]      # expand.grid: the index runs fastest
    assert rows[1] == "1\tA\t0.2\t0\t0.833333333333333\t0.2\tNA"
    assert rows[11] == "11\tA\t0.6\t0.2\t0.833333333333333\t0.8\tFALSE"       # 3 / 5 + 1 / 5 is 0.8, not above it
    assert rows[50] == "50\tA\t0.8\t0.2\t0.833333333333333\t1\tNA"
    assert rows[50 + 11] == "11\tB\t0.166666666666667\t0.333333333333333\t1\t0.5\tFALSE"
    assert rows[100 + 11] == "11\tC\tNaN\tNaN\t0\tNaN\tNA"                     # TRUE & NA is NA
    assert text["sp_snvFreq_fixed.tab"] == ("sampleID\tpropPass\tpropSuffCov\tsampleUsedForMedoidDefn\tpropHomogStrict\tselectedForDiscovery\n"
                                            "A\t0.8\t0.833333333333333\tFALSE\t0.6\tFALSE\n"
                                            "B\t0.5\t1\tFALSE\t0.333333333333333\tFALSE\n"
                                            "C\tNaN\t0\tNA\tNaN\tFALSE\n")
    assert result == [3, 6, 11, 0, 0, 1, 0, 0]
    text, result = model.files(["A", "B", "C"], HAND, "sp", min_prop_homog_snv=0.6)
    # the plot's rule is > on propPass (A: 0.8 > 0.6), the selection's is >= on propHomogStrict (A: 0.6 >= 0.6 holds; under > it would not)
    assert text["sp_snvFreq_fixed.tab"].split("\n")[1:4] == ["A\t0.8\t0.833333333333333\tTRUE\t0.6\tTRUE", "B\t0.5\t1\tFALSE\t0.333333333333333\tFALSE",
                                                             "C\tNaN\t0\tNA\tNaN\tFALSE"]
    assert result == [3, 6, 11, 1, 1, 1, 0, 0]
    text, result = model.files(["A", "B", "C"], HAND, "sp", max_prop_reads_non_homog=0.29)
    assert all(r.endswith("\tNA") for r in text["sp_snvFreq_cutoffs.tab"].split("\n")[1:151])
    # band (29, 71): A has 0, 5, 10, 95 outside = 4 / 5; B has 100, 90, 0.5 = 3 / 6
    assert text["sp_snvFreq_fixed.tab"].split("\n")[1:4] == ["A\tNA\tNA\tNA\t0.8\tTRUE", "B\tNA\tNA\tNA\t0.5\tFALSE", "C\tNA\tNA\tNA\tNaN\tFALSE"]
    assert result == [3, 6, 0, 0, 1, 1, 0, 0]


def test_the_class_form_is_the_literal_comparisons():
    """x <= k iff ceil(x) <= k and x >= 100 - k iff 100 - floor(x) <= k, on every double next to a cutoff and on 10^5 random cells."""
    v = cases.EDGE_VALUES
    assert v.size == 165 and np.isnan(v).sum() == 1 and np.nanmin(v) == 0.0 and np.nanmax(v) == 100.0
    for k in list(range(0, 52)) + [99, 100]:
        near = v[np.abs(v - k) < 1e-9]
        # 0.07 * 100 is the double above 7 and 0.29 * 100 the double below 29: each is in the list twice
        assert near.size == (2 if k in (0, 100) else 4 if k in (7, 29) else 3) and (near == k).sum() == 1, k
    assert 0.07 * 100 == np.nextafter(7.0, np.inf) and 0.29 * 100 == np.nextafter(29.0, -np.inf)
    t = cases.edge_table(400, 7)
    assert len({t[:, s].tobytes() for s in range(7)}) == 7 and (t[:, 5] == 0.0).all() and (t[:, 6] == 100.0).all() and np.isnan(t[:, 5:7]).sum() == 0
    for table in (t, cases.edge_table(331, 513)[:, 160:], np.random.default_rng(5).random((100000, 1)) * 100.0,
                  np.round(np.random.default_rng(6).random((100000, 1)), 4) * 100.0):
        c = model.counts(table)
        low, high = model.class_counts(table)
        assert (low == c["low"]).all() and (high == c["high"]).all()
        assert (c["low"][:, -1] + c["high"][:, -1] <= c["covered"]).all()
    wide = cases.edge_table(3, 513)
    assert len({wide[:, s].tobytes() for s in range(513) if s % 61 not in cases.CONSTANT}) == 513 - sum(1 for s in range(513) if s % 61 in cases.CONSTANT)
    assert np.isnan(wide[:, 7]).all() and np.isnan(wide[:, 68]).all()


def test_the_thresholds_in_double():
    assert model.matching_cutoff(0.1) == 11 and model.matching_cutoff(0.07) == 8 and 0.07 * 100 != 7.0 and 0.07 * 100 + 1 == 8.0
    assert model.matching_cutoff(0.29) == 0 and 0.29 * 100 + 1 == 29.999999999999996
    assert model.matching_cutoff(0.075) == 0
    assert model.matching_cutoff(0.0) == 1 and model.matching_cutoff(0.49) == 50 and model.matching_cutoff(0.5) == 0 and model.matching_cutoff(1.0) == 0
    assert model.strict_band(0.1) == (10.0, 90.0) == cases.BANDS[0]
    assert model.strict_band(0.07) == cases.BANDS[1]
    lo, hi = model.strict_band(0.9)                          # the fold: 1 - 0.9 is not 0.1
    assert lo == (1.0 - 0.9) * 100.0 and lo < 10.0 and hi == 100.0 - lo and lo != model.strict_band(0.1)[0]
    assert model.strict_band(0.56) == cases.BANDS[2]          # hi / lo of the folded 0.43999999999999995
    assert model.strict_band(0.5) == (50.0, 50.0)


def test_the_stage_tables_exercise_both_rules():
    """The 37 x 1100 table of the file-stage tests: some samples pass and some fail under each rule, and one sample has no covered cell."""
    for i in range(len(cases.STAGE_OPTS)):
        _, result = cases.stage_files(i)
        assert result[:2] == [37, 1100] and result[5] == 1
        assert 0 < result[4] < 36
    assert cases.stage_files(0)[1][2] == 11 and 0 < cases.stage_files(0)[1][3] < 36
    assert cases.stage_files(1)[1][2] == 8 and cases.stage_files(2)[1][2:4] == [0, 0]


def test_the_library_declares_the_defaults_and_the_geometry():
    import ctypes as C
    from metasnv_amd import _lib, subpopr
    o = _lib.SnvFreqOpts(9.0, 9.0, (C.c_int32 * 2)(7, 7))
    _lib.lib.msnv_snvfreq_opts_default(C.byref(o))
    assert C.sizeof(o) == 24 and (o.max_prop_reads_non_homog, o.min_prop_homog_snv, list(o.reserved)) == (0.1, 0.8, [0, 0])
    rows, lanes = subpopr.freq_curves_geometry()
    assert lanes == 64 and rows >= 1 and 4 * 100 * lanes <= 48 * 1024      # a hundred u32 counters a lane within the static LDS limit; u32 holds any slab below 2^32 rows


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_launcher_refuses_to_run_without_a_gpu(tmp_path):
    import os
    from metasnv_amd.subpopr import snv_freq_subpops_main
    path = tmp_path / "sp.filtered.freq"
    with pytest.raises(SystemExit) as err:
        snv_freq_subpops_main([str(path), str(tmp_path / "out")])
    assert "missing input file" in str(err.value)
    cases.write_freq(str(path), cases.sample_names(3), cases.random_unit_table(1, 4, 3))
    with pytest.raises(SystemExit) as err:
        snv_freq_subpops_main([str(path), str(tmp_path / "out"), "--fix-read-threshold", "0.07"])
    assert "no CPU fallback" in str(err.value)
    assert os.listdir(str(tmp_path)) == ["sp.filtered.freq"]
