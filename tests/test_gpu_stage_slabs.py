"""The row-slab loops of the file stages (csrc/stagedev.h: slab_rows) with more than one slab.  At test sizes a table always fits the device
whole, so MSNV_STAGE_SLAB_ROWS caps a slab at a few rows: dev_genotype_rows, dev_gene_corr and dev_freq_bands then walk several slabs, the
last one ragged.  Every case compares the run under the knob with the same call without it, bit for bit, and both with the CPU model the
stage's own tests use.  Also here: the kernel time a stage reports is that call's own."""
import ctypes as C

import numpy as np
import pytest

import distmodel
import genecorrcases
import genecorrmodel
import genotypecases
import genotypemodel
import pamcases
from metasnv_amd import core, subpopr, _lib
from metasnv_amd._lib import MsnvError, EDOMAIN, CLUSTER_TOO_FEW
from test_gpu_cluster import run_stage
from test_gpu_genecorr import COEF_BOUND

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def with_knob(monkeypatch, rows, call):
    if rows is None:
        monkeypatch.delenv("MSNV_STAGE_SLAB_ROWS", raising=False)
    else:
        monkeypatch.setenv("MSNV_STAGE_SLAB_ROWS", str(rows))
    return call()


# ---------------------------------------------------------------------------------------------- genotype rows
def genotype_case():
    """6 sample columns in 2 clusters of 3; 13 rows: 8 planted (each selects a cluster, every second one flipped), 4 of noise, and last a row
    whose cluster means differ by exactly the threshold: the kernel flags it and the host decides it."""
    table, clust = genotypecases.planted_genotypes(6, 2, 4, 4, 5)
    table = np.concatenate([table, [np.where(clust == 1, 90.0, 10.0)]])
    assert table.shape == (13, 6) and sorted(clust.tolist()) == [1, 1, 1, 2, 2, 2]
    return table, clust


@pytest.mark.parametrize("slab", [1, 5, 13, 100])
def test_genotype_rows_in_slabs(ctx, monkeypatch, slab):
    table, clust = genotype_case()
    select, flip, near = genotypemodel.genotype_rows(table, clust, 80.0)
    assert np.count_nonzero(select) >= 8 and np.count_nonzero(flip) >= 4 and near[12] and select[12] == 0      # the flagged row: in the last slab
    whole = with_knob(monkeypatch, None, lambda: subpopr.genotype_rows(ctx, table, clust, 80.0))
    got = with_knob(monkeypatch, slab, lambda: subpopr.genotype_rows(ctx, table, clust, 80.0))
    for res in (whole, got):
        assert res["select"].tolist() == select.tolist() and res["flip"].tolist() == flip.tolist()
        assert res["n_rechecked"] == int(near.sum()) and res["n_rechecked"] >= 1
        assert res["ms_kernel"] > 0


# ---------------------------------------------------------------------------------------------- gene correlation
def genecorr_case(last_cell):
    """2 cluster rows (one cluster and the column sums), 10 gene rows, 8 samples; gene row 9 holds `last_cell` in its last column."""
    clust, genes = genecorrcases.make_case(8, 1, 77)
    row9 = np.exp(np.random.RandomState(9).normal(0.0, 2.0, 8))
    row9[7] = last_cell
    genes = np.concatenate([genes, [row9]])
    assert clust.shape == (2, 8) and genes.shape == (10, 8)
    return clust, genes


@pytest.mark.parametrize("slab", [4, 10])
def test_gene_corr_in_slabs(ctx, monkeypatch, slab):
    """At 4 the matrix is not resident: the second walk uploads every slab again.  The smallest positive cell lies in gene row 9, the last
    slab: the pseudocount is right only if the first walk finished every slab before a logarithm was taken."""
    clust, genes = genecorr_case(1e-9)
    assert genes[genes > 0].min() == 1e-9 and genes[:9][genes[:9] > 0].min() > 1e-6
    want = genecorrmodel.gene_correlations(clust, genes)
    whole = with_knob(monkeypatch, None, lambda: subpopr.gene_correlations(ctx, clust, genes))
    got = with_knob(monkeypatch, slab, lambda: subpopr.gene_correlations(ctx, clust, genes))
    assert got["pseudocount"] == whole["pseudocount"] == want["pseudocount"] == 1e-9 / 1000.0
    for key in ("rho", "r", "valid"):
        assert got[key].tobytes() == whole[key].tobytes(), key
    assert (got["valid"] == want["valid"]).all() and got["valid"][:, 9].all()
    ok = want["valid"]
    assert np.isnan(got["rho"][~ok]).all() and np.isnan(got["r"][~ok]).all()
    d_rho, d_r = np.abs(got["rho"][ok] - want["rho"][ok]).max(), np.abs(got["r"][ok] - want["r"][ok]).max()
    print("slab %d: worst |rho - model| %.3g, worst |r - model| %.3g (bound %.0e)" % (slab, d_rho, d_r, COEF_BOUND))
    assert d_rho <= COEF_BOUND and d_r <= COEF_BOUND
    assert got["ms_kernel"] > 0 and whole["ms_kernel"] > 0


@pytest.mark.parametrize("slab", [4, 10])
def test_gene_corr_refuses_a_negative_cell_in_the_last_slab(ctx, monkeypatch, slab):
    clust, genes = genecorr_case(-0.5)
    for rows in (None, slab):
        with pytest.raises(MsnvError) as e:
            with_knob(monkeypatch, rows, lambda: subpopr.gene_correlations(ctx, clust, genes))
        assert e.value.code == EDOMAIN and "a negative, NaN or infinite abundance" in str(e.value)


# ---------------------------------------------------------------------------------------------- frequency bands
def test_frequency_bands_in_slabs(ctx, monkeypatch, tmp_path):
    """test_gpu_cluster.py::test_stage_medoid_definition_fails' table with 20 positions: slabs of 7, 7 and 6.  run_stage compares every file
    and the result with pammodel."""
    names = pamcases.sample_names(9)
    table = pamcases.planted_freqs(9, 2, 6, n_pos=20)
    table[:4, ::2] = 50.0
    dist = pamcases.manhattan(table)
    whole, files_whole = with_knob(monkeypatch, None, lambda: run_stage(ctx, tmp_path / "whole", names, dist, freq=(names, table.T)))
    got, files = with_knob(monkeypatch, 7, lambda: run_stage(ctx, tmp_path / "slabs", names, dist, freq=(names, table.T)))
    assert got["status"] == CLUSTER_TOO_FEW and sorted(files) == ["clustMedoidDefnFailed/sp_freq_composition.tab"]
    assert files == files_whole
    assert {k: v for k, v in got.items() if k != "ms_kernel"} == {k: v for k, v in whole.items() if k != "ms_kernel"}
    assert got["ms_kernel"] > 0 and whole["ms_kernel"] > 0


# ---------------------------------------------------------------------------------------------- kernel time
def test_dist_reports_each_call_its_own_kernel_time(ctx, tmp_path):
    names, text = distmodel.make_table(3, 300, 5)
    path = str(tmp_path / "t.filtered.freq")
    with open(path, "w") as f:
        f.write(text)
    times = []
    for start in (0.0, 0.0, 1e9):                                 # fresh variables, and one that holds a number already
        ms = C.c_double(start)
        _lib.check(_lib.lib.msnv_dist_file(ctx._h, path.encode(), (path + ".mann").encode(), (path + ".allele").encode(), 0.6, None, None, C.byref(ms)))
        times.append(ms.value)
    print("kernel ms of three calls:", times)
    assert all(0 < t < 1e4 for t in times)                         # a table of 300 x 5 cells: nowhere near ten seconds, and not a sum with 1e9
