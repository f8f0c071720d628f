"""tests/genecorrmodel.py -- the numpy restatement of subpopr's correlateSubpopProfileWithGeneProfiles -- against the files the
reference wrote (tests/golden/subpopr/genecorr: documentation/exampleTutorial/exampleResults of the reference) and, where it is
installed, against scipy.  The gene table behind the example's result files is not vendored, so the coefficients cannot be
recomputed; the files still pin every derived column as a function of (estimate, nObs) or of their own p column, and the layout."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import genecorrcases as cases
import genecorrmodel as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_derived_columns_match_the_reference_output(method):
    """Every row of the fixture: its estimate and nObs in, statistic / p.value / conf.int.* / q.valueBH compared.  Bounds:
    genecorrcases.BOUNDS (10 x the distance of a scipy evaluation of the same formula from the fixture)."""
    _, cols = cases.read_fixture(method)
    assert len(cols["estimate"]) == 400 and set(cols["nObs"]) == {"150"}
    res = model.corr_stats(method, [float(x) for x in cols["estimate"]], 150)
    cases.check_against_fixture(method, res)
    q = model.bh([float(x) for x in cols["p.value"]])            # BH as a function of the file's own p column
    d = cases.distance("rel", q, [float(x) for x in cols["q.valueBH"]])
    print("%s q.valueBH from the fixture's p: worst rel distance %.3g (bound %.3g)" % (method, d, cases.BH_BOUND))
    assert d <= cases.BH_BOUND
    assert min(float(x) for x in cols["p.value"]) < 1e-40 or method == "spearman"      # the tail the bound is held in


@pytest.mark.parametrize("n_clusters", [1, 3])
@pytest.mark.parametrize("n_samples", cases.SAMPLE_SIZES + (8192,))
def test_coefficients_and_p_match_scipy(n_samples, n_clusters):
    stats = pytest.importorskip("scipy.stats")
    clust, genes = cases.make_case(n_samples, n_clusters, 1000 + n_samples)
    res = model.gene_correlations(clust, genes)
    assert res["pseudocount"] == genes[genes > 0].min() / 1000.0
    n_valid = 0
    for c in range(clust.shape[0]):
        for g in range(genes.shape[0]):
            ok = clust[c].max() != clust[c].min() and genes[g].max() != genes[g].min()
            assert res["valid"][c, g] == ok
            if not ok:
                continue
            n_valid += 1
            rho, p_rho = stats.spearmanr(clust[c], genes[g])
            r, p_r = stats.pearsonr(np.log10(clust[c] + res["pseudocount"]), np.log10(genes[g] + res["pseudocount"]))
            assert abs(res["rho"][c, g] - rho) <= 1e-11 and abs(res["r"][c, g] - r) <= 1e-11, (c, g)
            if n_samples > 3:                                     # scipy's own p at the model's estimate
                for method, est, p_ref in (("spearman", res["rho"][c, g], p_rho), ("pearson", res["r"][c, g], p_r)):
                    p = 0.0 if abs(est) >= 1 else model.t_two_sided(model.t_statistic(method, est, n_samples - 2.0), n_samples - 2.0)
                    # p moves with the estimate: d ln p / d est is below n / (1 - est^2) in size
                    slack = 1e-11 * n_samples / max(1e-300, 1.0 - est * est) if abs(est) < 1 else 0.0
                    assert abs(p - p_ref) <= (1.2e-12 + slack) * max(p_ref, 1e-300) + 1e-300, (c, g, p, p_ref)
    assert n_valid >= (clust.shape[0] - (n_clusters == 3)) * (genes.shape[0] - 1) - 2
    assert not res["valid"][:, cases.INVALID_GENE].any()
    assert abs(res["rho"][0, 5] - 1.0) <= 1e-11 and abs(res["r"][0, 5] - 1.0) <= 1e-11 and abs(res["rho"][0, 6] + 1.0) <= 1e-11


def test_average_ranks_and_bh_by_hand():
    assert model.average_ranks([3.0, 1.0, 3.0, 0.0, 3.0, 1.0]).tolist() == [5.0, 2.5, 5.0, 1.0, 5.0, 2.5]
    p = np.array([0.01, 0.04, 0.03, 0.04, 0.9])
    # sorted descending 0.9 0.04 0.04 0.03 0.01 at ranks 5 4 3 2 1: 0.9, 0.05, 0.0667 -> 0.05, 0.075 -> 0.05, 0.05
    assert np.allclose(model.bh(p), [0.05, 0.05, 0.05, 0.05, 0.9], rtol=1e-15, atol=0)
    assert model.bh(np.array([0.6, 0.9])).tolist() == [0.9, 0.9]


def test_edges_of_the_derived_columns():
    st = model.corr_stats("pearson", [1.0, -1.0, 0.0, 0.5, 0.5], [10, 10, 10, 3, 4])
    assert st["statistic"][0] == math.inf and st["statistic"][1] == -math.inf and st["statistic"][2] == 0.0
    assert st["p_value"][:3].tolist() == [0.0, 0.0, 1.0]
    assert math.isnan(st["conf_low"][3]) and math.isnan(st["conf_high"][3])
    # n = 3: one degree of freedom, p = 1 - 2 atan(t) / pi with t = 0.5 / sqrt(0.75); n = 4: p = 1 - |r| exactly
    assert abs(st["p_value"][3] - (1.0 - 2.0 * math.atan(0.5 / math.sqrt(0.75)) / math.pi)) < 1e-15
    assert abs(st["p_value"][4] - 0.5) < 1e-15
    assert abs(st["conf_low"][4] - math.tanh(math.atanh(0.5) - model.QNORM_975)) < 1e-15
    sp = model.corr_stats("spearman", [1.0, -1.0], 5)
    assert sp["statistic"].tolist() == [0.0, 40.0] and sp["p_value"].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_writer_reproduces_the_fixtures_layout(method):
    """Header byte for byte, the column count of every row, the constant cells; every number the writer prints reads back to the
    same double and no exponent is zero-padded.  Byte identity of the numbers with readr is not claimed."""
    header, cols = cases.read_fixture(method)
    first_line = open(cases.FIXTURE[method]).readline()
    n = len(cols["estimate"])
    res = model.corr_stats(method, [float(x) for x in cols["estimate"]], 150)
    rows = []
    for i in range(n):
        w = {"gene": cols["geneFamily"][i], "cluster": cols["cluster"][i], "statistic": res["statistic"][i], "p": res["p_value"][i],
             "estimate": float(cols["estimate"][i]), "n_obs": 150, "q": res["q_value"][i]}
        if method == "pearson":
            w["lo"], w["hi"] = res["conf_low"][i], res["conf_high"][i]
        rows.append(w)
    text = model.table_text(method, rows)
    lines = text.split("\n")
    assert lines[0] + "\n" == first_line and lines[-1] == "" and len(lines) == n + 2
    numeric = [h for h in header if h not in ("geneFamily", "cluster", "alternative", "method", "conf.int")]
    exponents = 0
    for i, ln in enumerate(lines[1:-1]):
        f = ln.split("\t")
        assert len(f) == len(header)
        got = dict(zip(header, f))
        for h in ("geneFamily", "cluster", "null.value", "alternative", "method", "nObs") + (("conf.int",) if method == "pearson" else ()):
            assert got[h] == cols[h][i], (i, h)
        for h in numeric:
            assert not re.search(r"e[+-]?0\d", got[h]), got[h]
            exponents += "e" in got[h]
        back = {"statistic": "statistic", "p.value": "p", "estimate": "estimate", "q.valueBH": "q", "conf.int.low": "lo", "conf.int.high": "hi"}
        for h, key in back.items():
            if h in got:
                assert float(got[h]) == rows[i][key], (i, h)
    assert exponents > 0
    assert model.r_number(1e-8) == "1e-8" and model.r_number(1.5e-10) == "1.5e-10" and model.r_number(float("nan")) == "NA"
    assert model.r_number(float("inf")) == "Inf" and model.r_number(-float("inf")) == "-Inf" and model.r_number(0.1) == "0.1"


def test_selection_rules_on_a_hand_made_table():
    def row(gene, cluster, est, q, n=20):
        return {"gene": gene, "cluster": cluster, "estimate": est, "q": q, "n_obs": n}
    pear = [row("gA", "1", 0.9, 0.01), row("gA", "2", 0.1, 0.5), row("gA", "-1", 0.3, 0.2),      # specific to cluster 1
            row("gB", "1", 0.9, 0.01), row("gB", "2", 0.5, 0.01), row("gB", "-1", 0.3, 0.2),      # cluster 2 neither: only cluster 1 is listed ... but nothing fails
            row("gC", "1", 0.9, 0.01), row("gC", "2", 0.1, 0.5), row("gC", "-1", 0.95, 0.001),    # species gene: forced not correlated
            row("gD", "1", 0.9, 0.2), row("gD", "2", 0.1, 0.5), row("gD", "-1", 0.0, 1.0)]       # q too high
    spear = [dict(w, estimate={0.9: 0.7, 0.95: 0.7}.get(w["estimate"], w["estimate"])) for w in pear]
    species, clusters = model.select_specific(pear, spear)
    assert species == [("gC", "-1", True, False)]
    assert clusters == [("gA", "1", True, False), ("gA", "2", False, True)]
    few = [dict(w, n_obs=9) for w in pear]
    assert model.select_specific(few, [dict(w, n_obs=9) for w in spear]) == ([], [])


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_launcher_refuses_to_run_without_a_gpu(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(cases.ABUND, str(out / "sp_allClust_relativeAbund.tab"))
    genes = tmp_path / "genes.tsv"
    genes.write_text("id\tm1.insilicoRefs.unique.sorted.bam\ng1\t1\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "correlateSubpopProfileWithGeneProfiles.py"), "sp", str(out) + "/", str(genes), "Genes"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert sorted(os.listdir(str(out))) == ["sp_allClust_relativeAbund.tab"]
