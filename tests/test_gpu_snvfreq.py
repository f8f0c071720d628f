"""The counts behind subpopr's SNV-frequency plots on the device (csrc/snvfreq_k.hip, csrc/snvfreq.cpp) against tests/snvfreqmodel.py.  Every
comparison with the model is exact: integers equal, files byte-equal.

The kernel's two tile constants are FREQ_CURVE_ROWS (the rows one block walks, 1024) and FREQ_CURVE_LANES (the sample columns of a block, one
wavefront of 64), both in csrc/device.h; the tests read them from the library (msnv_freq_curves_geometry) as ROWS and LANES.  The widths sit on both
sides of one block, of four and of eight (63 / 64 / 65, 255 / 256 / 257, 513, and a single column); the row counts are 0, 1, and one short of, exactly
at and one past ROWS and 2 ROWS.  The constant columns (all 0.0, all 100.0) put every cell of a slab into one counter: at ROWS + 1 rows a
per-block counter has taken a whole slab, and at 65 537 rows a 16-bit one would have wrapped."""
import os

import numpy as np
import pytest

import snvfreqcases as cases
import snvfreqmodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EINVAL
from metasnv_amd.subpopr import freq_curves, freq_curves_geometry, snv_freq_file, snv_freq_subpops_main

pytestmark = pytest.mark.gpu
ROWS, LANES = freq_curves_geometry()
ROW_COUNTS = (0, 1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1)
KEYS = ("low", "high", "covered", "strict")


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def same(got, want, S):
    for key in KEYS:
        assert got[key].dtype == np.uint64 and got[key].shape == want[key][:S].shape, key
        assert (got[key] == want[key][:S]).all(), (key, np.argwhere(got[key] != want[key][:S])[:4].tolist())


def test_the_geometry_is_the_documented_one():
    assert (ROWS, LANES) == (1024, 64)                          # the module docstring and KERNELS.md name these values


@pytest.mark.parametrize("S", cases.WIDTHS)
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_counts_on_the_edge_table(ctx, n, S):
    got = freq_curves(ctx, cases.edge_table(n, S))
    same(got, cases.edge_counts(n), S)
    assert got["low"].shape == (S, 50) and got["high"].shape == (S, 50)
    if n == 0:
        assert not any(got[key].any() for key in KEYS)
    else:
        assert got["ms_kernel"] > 0


@pytest.mark.parametrize("n", (ROWS + 1, 65537))
def test_constant_columns_past_a_slab(ctx, n):
    t = cases.edge_table(n, 8)
    assert (t[:, 5] == 0.0).all() and (t[:, 6] == 100.0).all() and np.isnan(t[:, 7]).all()
    got = freq_curves(ctx, t)
    assert got["low"][5].tolist() == [n] * 50 and got["high"][5].tolist() == [0] * 50          # every cell in low class 0
    assert got["high"][6].tolist() == [n] * 50 and got["low"][6].tolist() == [0] * 50          # every cell in high class 0
    assert got["covered"].tolist()[5:] == [n, n, 0] and got["strict"].tolist()[5:] == [n, n, 0]
    assert not got["low"][7].any() and not got["high"][7].any()
    same(got, model.counts(t), 8)


@pytest.mark.parametrize("S", (65, 257))
def test_row_slabs_leave_the_same_counts(ctx, monkeypatch, S):
    n = 2 * ROWS + 1
    t = cases.edge_table(n, S)
    monkeypatch.delenv("MSNV_STAGE_SLAB_ROWS", raising=False)
    whole = freq_curves(ctx, t)
    same(whole, cases.edge_counts(n), S)
    assert whole["ms_kernel"] > 0
    for slab in (1, 7, n + 1):                                 # 7: 292 slabs of 7 and a last one of 5
        monkeypatch.setenv("MSNV_STAGE_SLAB_ROWS", str(slab))
        got = freq_curves(ctx, t)
        assert got["ms_kernel"] > 0, slab
        for key in KEYS:
            assert got[key].tobytes() == whole[key].tobytes(), (slab, key)


@pytest.mark.parametrize("band", cases.BANDS)
def test_strict_bands(ctx, band):
    n, S = ROWS + 1, 257
    got = freq_curves(ctx, cases.edge_table(n, S), strict_lo=band[0], strict_hi=band[1])
    same(got, cases.edge_counts(n, band), S)
    assert (got["low"] == cases.edge_counts(n)["low"][:S]).all()        # the band moves the strict count alone


# ---------------------------------------------------------------------------------------------- the stage on files
def write_stage_table(tmp_path):
    path = str(tmp_path / "sp.filtered.freq")
    cases.write_freq(path, cases.sample_names(cases.STAGE_SHAPE[1]), cases.stage_table())
    return path


def result_list(res):
    return [res["n_samples"], res["n_rows"], res["cutoff_index"], res["n_used_for_medoid_defn"], res["n_selected"], res["n_uncovered"], 0, 0]


def check_files(out, files):
    directory = os.path.join(out, "snvFreqPlots")
    assert sorted(os.listdir(directory)) == sorted(files)
    for name, text in files.items():
        assert open(os.path.join(directory, name)).read() == text, name


@pytest.mark.parametrize("which", range(len(cases.STAGE_OPTS)))
def test_stage_writes_the_models_files(ctx, tmp_path, which):
    path = write_stage_table(tmp_path)
    files, result = cases.stage_files(which)
    out = str(tmp_path / "out")                                # neither out nor out/snvFreqPlots exists
    res = snv_freq_file(ctx, path, out, **cases.STAGE_OPTS[which])
    check_files(out, files)
    assert result_list(res) == result and res["ms_kernel"] > 0
    if which == 2:                                             # -x 0.29 matches no cutoff: NA columns, the last two filled
        rows = [r.split("\t") for r in files["sp_snvFreq_fixed.tab"].splitlines()[1:]]
        assert all(r[1:4] == ["NA", "NA", "NA"] and r[4] != "NA" and r[5] in ("TRUE", "FALSE") for r in rows) and res["cutoff_index"] == 0
    res = snv_freq_file(ctx, path, out, species="sp", **cases.STAGE_OPTS[which])      # into the directory that now exists
    check_files(out, files)
    assert result_list(res) == result


def refused(code, fn, *args, **kw):
    with pytest.raises(MsnvError) as err:
        fn(*args, **kw)
    assert err.value.code == code, err.value
    return str(err.value)


def test_cells_outside_the_scale_are_refused(ctx, tmp_path, monkeypatch):
    names = cases.sample_names(5)
    t = cases.random_unit_table(3, 20, 5)
    path = str(tmp_path / "sp.filtered.freq")
    for bad, old_version in ((1.5, True), (-0.5, False)):
        u = t.copy()
        u[19, 4] = bad                                         # the last row of the last slab: 20 rows are slabs of 7, 7 and 6
        cases.write_freq(path, names, u)
        for slab in (None, "7"):
            if slab is None:
                monkeypatch.delenv("MSNV_STAGE_SLAB_ROWS", raising=False)
            else:
                monkeypatch.setenv("MSNV_STAGE_SLAB_ROWS", slab)
            msg = refused(EDOMAIN, snv_freq_file, ctx, path, str(tmp_path / "out"))
            assert ("old version of metaSNV" in msg) == old_version, msg
    monkeypatch.delenv("MSNV_STAGE_SLAB_ROWS", raising=False)
    assert not os.path.exists(str(tmp_path / "out" / "snvFreqPlots" / "sp_snvFreq_cutoffs.tab"))
    e = cases.edge_table(ROWS + 1, 65)
    for bad in cases.OUTSIDE:                                  # the array entry is on the percent scale
        for p, s in ((0, 0), (ROWS, 64)):
            u = e.copy()
            u[p, s] = bad
            refused(EDOMAIN, freq_curves, ctx, u)
    same(freq_curves(ctx, e), cases.edge_counts(ROWS + 1), 65)


def test_options_outside_their_range_are_refused(ctx, tmp_path):
    path = str(tmp_path / "sp.filtered.freq")
    cases.write_freq(path, cases.sample_names(3), cases.random_unit_table(4, 6, 3))
    out = str(tmp_path / "out")
    for bad in (dict(max_prop_reads_non_homog=-0.01), dict(max_prop_reads_non_homog=1.01), dict(min_prop_homog_snv=-0.01), dict(min_prop_homog_snv=1.5),
                dict(max_prop_reads_non_homog=float("nan")), dict(min_prop_homog_snv=float("nan")), dict(reserved=(1, 0)), dict(reserved=(0, -1))):
        refused(EINVAL, snv_freq_file, ctx, path, out, **bad)
    assert not os.path.exists(out)
    for edge in (dict(max_prop_reads_non_homog=0.0, min_prop_homog_snv=0.0), dict(max_prop_reads_non_homog=1.0, min_prop_homog_snv=1.0)):
        assert snv_freq_file(ctx, path, out, **edge)["n_samples"] == 3
    refused(EINVAL, freq_curves, ctx, np.zeros((4, 2)), strict_lo=float("nan"))
    refused(EINVAL, freq_curves, ctx, np.zeros((4, 0)))


def test_the_launcher_writes_the_same_files(ctx, tmp_path, capsys):
    path = write_stage_table(tmp_path)
    for which, argv in ((0, []), (1, ["--fix-read-threshold", "0.07", "--fix-snv-threshold", "0.5"]), (2, ["--species", "sp", "--fix-read-threshold", "0.29"])):
        files, result = cases.stage_files(which)
        out = str(tmp_path / ("out%d" % which))
        capsys.readouterr()
        res = snv_freq_subpops_main([path, out] + argv)
        printed = capsys.readouterr().out
        check_files(out, files)
        assert result_list(res) == result
        assert printed.count("\n") == 1 and printed.startswith("Species sp: 37 samples, 1100 rows; ")
        assert (" %d pass the plot's rule" % result[3]) in printed and (" %d pass the selection rule" % result[4]) in printed, printed
    with pytest.raises(SystemExit) as err:
        snv_freq_subpops_main([str(tmp_path / "nowhere.freq"), str(tmp_path / "out")])
    assert "missing input file" in str(err.value)
    assert subpopr.snv_freq_subpops_main is snv_freq_subpops_main
