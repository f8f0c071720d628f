"""subpopr's correlateSubpopProfileWithGeneProfiles on the device (csrc/genecorr_k.hip, csrc/genecorr.cpp) against
tests/genecorrmodel.py and the files the reference wrote (tests/golden/subpopr/genecorr).

msnv_gc_gene_rows ranks one row per workgroup: P = the next power of two >= max(S, 64) elements in LDS, min(P, 1024) threads.
The sample counts are the sizes at which that form changes: 3 and 4 (the smallest cor.test takes), 63 / 64 / 65 (one wavefront,
one padded tile), 255 / 256 / 257 (four wavefronts), 1023 / 1024 / 1025 (every thread one element; then several per thread) and
the cap, 8192 (112 KiB of LDS)."""
import os
import shutil

import numpy as np
import pytest

import genecorrcases as cases
import genecorrmodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EFORMAT

pytestmark = pytest.mark.gpu
CAP = 8192

# rho and r are quotients of three fp64 sums of n <= 8192 centred terms: each sum errs by at most n 2^-53 = 9.1e-13 relative, the
# quotient sxy / sqrt(sxx syy) by under 4 x that = 3.6e-12; 1e-11 leaves about 2.7 x more.  (Holds for rows whose spread in log10 is
# at least 1e-3 of their magnitude: genecorrcases.make_case.)
COEF_BOUND = 1e-11


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n_clusters", [1, 3])
@pytest.mark.parametrize("n_samples", cases.SAMPLE_SIZES + (CAP,))
def test_coefficients_at_the_sizes_where_the_kernel_changes_form(ctx, n_samples, n_clusters):
    clust, genes = cases.make_case(n_samples, n_clusters, 1000 + n_samples)
    want = model.gene_correlations(clust, genes)
    got = subpopr.gene_correlations(ctx, clust, genes)
    assert got["pseudocount"] == want["pseudocount"]
    assert (got["valid"] == want["valid"]).all()
    assert not got["valid"][:, cases.INVALID_GENE].any() and got["valid"][0].sum() == cases.N_GENES - 1
    if n_clusters == 3:
        assert not got["valid"][2].any()                           # the constant cluster vector
    ok = want["valid"]
    assert np.isnan(got["rho"][~ok]).all() and np.isnan(got["r"][~ok]).all()
    d_rho, d_r = np.abs(got["rho"][ok] - want["rho"][ok]).max(), np.abs(got["r"][ok] - want["r"][ok]).max()
    print("S=%d K=%d: worst |rho - model| %.3g, worst |r - model| %.3g (bound %.0e)" % (n_samples, n_clusters, d_rho, d_r, COEF_BOUND))
    assert d_rho <= COEF_BOUND and d_r <= COEF_BOUND
    assert abs(got["rho"][0, 5] - 1.0) <= COEF_BOUND and abs(got["r"][0, 5] - 1.0) <= COEF_BOUND      # the row equal to cluster 0
    assert abs(got["rho"][0, 6] + 1.0) <= COEF_BOUND                                                  # its mirror image
    assert got["ms_kernel"] > 0


def test_sample_counts_outside_the_domain_are_refused(ctx):
    for s in (CAP + 1, 2):
        with pytest.raises(MsnvError) as e:
            subpopr.gene_correlations(ctx, np.ones((2, s)), np.ones((3, s)))
        assert e.value.code == EDOMAIN
        if s > CAP:
            assert str(CAP) in str(e.value)
    with pytest.raises(MsnvError) as e:                            # no cell above 0: no pseudocount
        subpopr.gene_correlations(ctx, np.arange(8.0).reshape(1, 8), np.zeros((2, 8)))
    assert e.value.code == EDOMAIN
    with pytest.raises(MsnvError) as e:
        subpopr.gene_correlations(ctx, np.arange(8.0).reshape(1, 8), np.array([[1.0, 2, 3, 4, 5, 6, 7, np.nan]]))
    assert e.value.code == EDOMAIN


@pytest.mark.parametrize("n_samples", [5, 65, 1025, CAP])
def test_ranks_are_exact_on_integer_rows_without_ties(ctx, n_samples):
    """Permutations of 0 .. S-1: every rank is an integer, every centred product a multiple of 1/4 and every sum below 2^53, so
    sxy, sxx and syy are exact and rho is one correctly rounded quotient -- the device's must equal the model's bit for bit."""
    rnd = np.random.RandomState(n_samples)
    clust = np.array([rnd.permutation(n_samples) for _ in range(3)], dtype=np.float64)
    genes = np.array([rnd.permutation(n_samples) for _ in range(7)] + [clust[1], clust[1][::-1].max() - clust[1]], dtype=np.float64)
    want = model.gene_correlations(clust, genes)
    got = subpopr.gene_correlations(ctx, clust, genes)
    assert got["valid"].all() and got["pseudocount"] == 0.001
    assert (got["rho"] == want["rho"]).all()
    assert got["rho"][1, 7] == 1.0 and got["rho"][1, 8] == -1.0


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_derived_columns_against_the_reference_output(ctx, method):
    """The fixture's 400 estimates (nObs 150) in, its statistic / p.value / conf.int.* / q.valueBH compared: within 10 x the distance
    of a scipy evaluation from the fixture (genecorrcases.BOUNDS); q additionally against the model's BH of the device's own p.
    Measured worst cases: MEASURED.md, "Gene-profile correlations"."""
    _, cols = cases.read_fixture(method)
    got = subpopr.corr_stats(ctx, method, [float(x) for x in cols["estimate"]], 150)
    cases.check_against_fixture(method, got)
    d = cases.distance("rel", got["q_value"], model.bh(got["p_value"]))
    print("%s q.valueBH against BH of the device's own p: worst rel distance %.3g (bound %.3g)" % (method, d, cases.BH_BOUND))
    assert d <= cases.BH_BOUND


def test_derived_columns_at_their_edges(ctx):
    est, n = [1.0, -1.0, 0.0, 0.5, 0.5, -0.25, 0.999999], [10, 10, 10, 3, 4, 3, 8192]
    got, want = subpopr.corr_stats(ctx, "pearson", est, n), model.corr_stats("pearson", est, n)
    assert got["statistic"][0] == np.inf and got["statistic"][1] == -np.inf and got["statistic"][2] == 0.0
    assert got["p_value"][:3].tolist() == [0.0, 0.0, 1.0]
    assert np.isnan(got["conf_low"][[3, 5]]).all() and np.isnan(got["conf_high"][[3, 5]]).all()          # n = 3: NA interval
    assert got["conf_low"][0] == 1.0 and got["conf_high"][1] == -1.0
    assert abs(got["p_value"][4] - 0.5) <= 1e-15                     # n = 4: p = 1 - |r|
    for k, bound in (("statistic", 3.9e-15), ("p_value", 1.14e-12), ("q_value", 1.14e-12)):      # genecorrcases.BOUNDS, against the model
        assert cases.distance("rel", got[k][2:], want[k][2:]) <= bound, k
    assert cases.distance("abs", got["conf_low"][[2, 4, 6]], want["conf_low"][[2, 4, 6]]) <= 2.2e-15
    sp, sw = subpopr.corr_stats(ctx, "spearman", [1.0, -1.0, 0.0, 0.3], [5, 5, 3, 4]), model.corr_stats("spearman", [1.0, -1.0, 0.0, 0.3], [5, 5, 3, 4])
    assert sp["statistic"].tolist() == sw["statistic"].tolist() and sp["p_value"][:3].tolist() == [0.0, 0.0, 1.0]
    assert "conf_low" not in sp
    with pytest.raises(MsnvError) as e:
        subpopr.corr_stats(ctx, "pearson", [0.5], 2)
    assert e.value.code == EDOMAIN


@pytest.mark.parametrize("n_rows", [3, 2048, 2049, 5000])
def test_bh_against_the_model_with_tied_p_values(ctx, n_rows):
    """One table of 3 rows, one sort tile exactly (2048), one row more, and 5000 rows (padded to 8192: four tiles merged through
    global memory).  The estimates are drawn from 40 values, so most p-values are tied.  q is a chain of exact minima over
    (N / rank) p, the same operations in the model: equal bit for bit given the device's own p."""
    rnd = np.random.RandomState(n_rows)
    est = rnd.choice(np.round(rnd.uniform(-0.9, 0.9, 40), 3), n_rows)
    got = subpopr.corr_stats(ctx, "spearman", est, 30)
    assert (got["q_value"] == model.bh(got["p_value"])).all()
    assert cases.distance("rel", got["q_value"], model.corr_stats("spearman", est, 30)["q_value"]) <= 5.8e-13
    assert (got["q_value"] <= 1.0).all() and (got["q_value"] >= got["p_value"]).all()


# ------------------------------------------------------------------------------------------------ end to end
def _gene_table(path, suffix_cut=None, na_cell=False):
    """About 40 gene families over the fixture's abundance table (159 samples, 3 clusters): 149 of its samples (10 are missing) and 4
    columns it does not hold, '#' lines, an all-zero gene, genes planted as scale x one cluster's column (so the cluster file is
    not empty) and one planted on the species sum."""
    names, samples, ab = model.read_cluster_table(cases.ABUND)
    rnd = np.random.RandomState(5)
    use = [i for i in range(len(samples)) if i % 17 != 3]
    cols = [samples[i] for i in use]
    vals = {}
    for g in range(30):
        v = np.exp(rnd.normal(0.0, 1.5, len(use)))
        v[rnd.rand(len(use)) < 0.4] = 0.0
        vals["fam%02d" % g] = v
    vals["fam_zero"] = np.zeros(len(use))
    for k in range(3):
        vals["plant_c%d_a" % k] = 3.0 * ab[use, k]
        vals["plant_c%d_b" % k] = 0.02 * ab[use, k] * np.exp(rnd.normal(0.0, 0.05, len(use)))
    vals["plant_species"] = 11.0 * ab[use].sum(axis=1)
    vals["Zlast"] = np.round(rnd.uniform(0, 3, len(use)))
    extra = {0: "other1.bam", 40: "other2.bam", 90: "other3.bam", len(use): "other4.bam"}
    header, order = ["id"], []
    for j in range(len(use) + 1):
        if j in extra:
            header.append(extra[j]); order.append(None)
        if j < len(use):
            name = cols[j]
            header.append(name[:-len(suffix_cut)] if suffix_cut and name.endswith(suffix_cut) else name); order.append(j)
    lines = ["# gene family abundances", "\t".join(header), "# a comment between the rows"]
    for gi, (gene, v) in enumerate(vals.items()):
        cells = [model.r_number(v[j]) if j is not None else model.r_number(float(gi % 5)) for j in order]
        if na_cell and gene == "fam07":
            cells[12] = "NA"
        lines.append("\t".join([gene] + cells))
    open(path, "w").write("\n".join(lines) + "\n")


def _fields(text):
    return [ln.split("\t") for ln in text.split("\n")[:-1]]


def _compare_tables(method, got_text, want_text):
    got, want = _fields(got_text), _fields(want_text)
    assert got[0] == want[0] and len(got) == len(want) and len(got) > 50
    header = got[0]
    for h in header:
        i = header.index(h)
        a, b = [r[i] for r in got[1:]], [r[i] for r in want[1:]]
        if (method, h) in cases.BOUNDS:
            kind, bound = cases.BOUNDS[(method, h)]
            assert cases.distance(kind, [float(x) for x in a], [float(x) for x in b]) <= bound, h
        else:
            assert a == b, h                                        # names, labels, constants, nObs and the estimates themselves


def test_files_end_to_end_against_the_model(ctx, tmp_path, capsys):
    out = str(tmp_path / "out") + "/"
    os.makedirs(out)
    shutil.copy(cases.ABUND, out + "sp1_allClust_relativeAbund.tab")
    genes = str(tmp_path / "genes.tsv")
    _gene_table(genes)
    n = subpopr.correlate_gene_profiles_main(["sp1", out, genes, "Genes"])
    assert "Species sp1: Testing 3 clusters for correlation with 38 geneFamily groups in 149 samples" in capsys.readouterr().out
    labels, gene_names, clust, gm = model.prepare(out + "sp1_allClust_relativeAbund.tab", genes)
    assert labels == ["subsp1", "subsp2", "subsp3", "-1"] and "fam_zero" not in gene_names and clust.shape == (4, 149)
    own, counts, _ = model.run_files(out + "sp1_allClust_relativeAbund.tab", genes)
    dev = subpopr.gene_correlations(ctx, clust, gm)
    mixed, _, _ = model.run_files(out + "sp1_allClust_relativeAbund.tab", genes, corr=dev)      # the model's derived columns of the device's estimates
    got = {k: open(out + "sp1_corrGenes-" + k + ".tsv").read() for k in ("spearman", "pearson", "clusterSpecificGenes", "speciesSpecificGenes")}
    for method in ("pearson", "spearman"):
        _compare_tables(method, got[method], mixed[method])
        i = _fields(got[method])[0].index("estimate")
        a, b = [float(r[i]) for r in _fields(got[method])[1:]], [float(r[i]) for r in _fields(own[method])[1:]]
        assert cases.distance("abs", a, b) <= COEF_BOUND
    assert got["clusterSpecificGenes"] == own["clusterSpecificGenes"] and got["speciesSpecificGenes"] == own["speciesSpecificGenes"]
    assert got["speciesSpecificGenes"].count("\n") >= 2 and "plant_species\t-1\tTRUE\tFALSE\n" in got["speciesSpecificGenes"]
    for k in range(3):
        assert "plant_c%d_a\tsubsp%d\tTRUE\tFALSE\n" % (k, k + 1) in got["clusterSpecificGenes"]
    assert n == counts[3] >= 6

    # the same table with the suffix cut off the column names, and --sample-suffix: identical tables
    out2 = str(tmp_path / "out2") + "/"
    os.makedirs(out2)
    shutil.copy(cases.ABUND, out2 + "sp1_allClust_relativeAbund.tab")
    cut = str(tmp_path / "genes_cut.tsv")
    _gene_table(cut, suffix_cut=".insilicoRefs.unique.sorted.bam")
    with pytest.raises(SystemExit) as e:                           # without the suffix nothing overlaps: an error that names example ids
        subpopr.correlate_gene_profiles_main(["sp1", out2, cut, "Genes"])
    assert "No overlapping sample IDs" in str(e.value) and "m1.insilicoRefs.unique.sorted.bam" in str(e.value) and "other1.bam" in str(e.value)
    assert os.listdir(out2) == ["sp1_allClust_relativeAbund.tab"]
    assert subpopr.correlate_gene_profiles_main(["sp1", out2, cut, "Genes", "--sample-suffix", ".insilicoRefs.unique.sorted.bam"]) == n
    for k in got:
        assert open(out2 + "sp1_corrGenes-" + k + ".tsv").read() == got[k], k


def test_files_cluster_filter_and_refused_cells(ctx, tmp_path):
    names, samples, ab = model.read_cluster_table(cases.ABUND)
    genes = str(tmp_path / "genes.tsv")
    _gene_table(genes)
    # a fourth cluster seen in two samples only is left out; one seen in three stays (label: one leading X removed)
    lines = open(cases.ABUND).read().split("\n")
    rows = [lines[0] + "\tX7\tXX"] + [ln + "\t" + ("0.5" if i in (0, 5) else "0") + "\t" + ("0.25" if i in (1, 2, 8) else "0") for i, ln in enumerate(lines[1:]) if ln]
    wide = str(tmp_path / "wide.tab")
    open(wide, "w").write("\n".join(rows) + "\n")
    k, g, s, _ = subpopr.gene_corr_files(ctx, wide, genes, str(tmp_path / "w"))
    assert (k, g, s) == (4, 38, 149)
    labels = {r[1] for r in _fields(open(str(tmp_path / "w-pearson.tsv")).read())[1:]}
    assert labels == {"X", "subsp1", "subsp2", "subsp3", "-1"}
    want, _, _ = model.run_files(wide, genes)
    assert [r[:2] for r in _fields(open(str(tmp_path / "w-spearman.tsv")).read())] == [r[:2] for r in _fields(want["spearman"])]
    # no cluster in three samples: nothing is written, every count is 0
    none = str(tmp_path / "none.tab")
    open(none, "w").write("a\tb\n" + "".join("s%d\t%s\t0\n" % (i, "0.5" if i < 2 else "0") for i in range(6)))
    assert subpopr.gene_corr_files(ctx, none, genes, str(tmp_path / "n")) == (0, 0, 0, 0)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("n-")]
    # an NA cell in either table
    bad = str(tmp_path / "bad.tsv")
    _gene_table(bad, na_cell=True)
    with pytest.raises(MsnvError) as e:
        subpopr.gene_corr_files(ctx, cases.ABUND, bad, str(tmp_path / "b"))
    assert e.value.code == EFORMAT
    bad_ab = str(tmp_path / "bad.tab")
    open(bad_ab, "w").write(open(cases.ABUND).read().replace("\t0\t", "\tNA\t", 1))
    with pytest.raises(MsnvError) as e:
        subpopr.gene_corr_files(ctx, bad_ab, genes, str(tmp_path / "b"))
    assert e.value.code == EFORMAT
    # two samples in common: cor.test stops below three observations
    two = str(tmp_path / "two.tsv")
    open(two, "w").write("id\t%s\t%s\ng1\t1\t2\n" % (samples[0], samples[1]))
    with pytest.raises(MsnvError) as e:
        subpopr.gene_corr_files(ctx, cases.ABUND, two, str(tmp_path / "t"))
    assert e.value.code == EDOMAIN
