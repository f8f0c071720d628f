"""tests/profilemodel.py -- the numpy restatement of subpopr's writeSubpopsForAllSamples and writeSubpopAbundSpeciesAbund that tests/test_gpu_profile.py
judges the device by -- pinned on hand-worked tables, the exact text of every file and stat line, and the host-only abundance stage of the library
against it.  No GPU is needed; the two launchers are run as far as they go without one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import profilecases as cases
import profilemodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
FLIP = [False, True, False, False, True]                                # the rows of the G = 5 cases


def test_hand_worked_columns():
    rows = np.array([[0, 100, 100, 0, 50], [0, 100, 30, 60, 100]], dtype=np.float64).T
    assert model.flipped(rows, FLIP).T.tolist() == [[0, 0, 100, 0, 50], [0, 0, 30, 60, 0]]
    got = model.profile_columns(rows, FLIP)
    assert got["n_called"].tolist() == [5, 5] and got["n_eq0"].tolist() == [3, 3] and got["n_eq100"].tolist() == [1, 0]
    assert got["n_gt0"].tolist() == [2, 2] and got["n_ge5"].tolist() == [2, 2]
    assert got["mid_lo"].tolist() == [0, 0] and got["mid_hi"].tolist() == [0, 0]
    kept = model.summarise(rows, np.array(FLIP), 0.2)
    assert [(r[2], r[4], r[6], r[7], r[8]) for r in kept] == [(0.0, 0.4, 3, 1, 0), (0.0, 0.4, 3, 0, 0)]
    assert kept[0][1] == 30.0 and kept[1][1] == 18.0                    # means
    assert kept[0][3] == pytest.approx(np.std([0, 0, 100, 0, 50], ddof=1), rel=1e-15)


def test_median_of_an_even_count_and_of_nothing():
    got = model.profile_columns(np.array([[10, 20, NAN, 40, 30], [NAN] * 5, [NAN, NAN, 7, NAN, NAN], [-0.0, NAN, NAN, NAN, NAN]]).T, [False] * 5)
    assert got["n_called"].tolist() == [4, 0, 1, 1]
    assert (got["mid_lo"][0], got["mid_hi"][0]) == (20.0, 30.0) and model.r_mean([20.0, 30.0]) == 25.0
    assert np.isnan(got["mid_lo"][1]) and np.isnan(got["mid_hi"][1])
    assert (got["mid_lo"][2], got["mid_hi"][2]) == (7.0, 7.0)
    assert got["n_eq0"][3] == 1 and not np.signbit(got["mid_lo"][3])    # -0.0 counts as +0.0
    with pytest.raises(model.DomainError):
        model.profile_columns(np.array([[100.5]]), [False])
    with pytest.raises(model.DomainError):
        model.profile_columns(np.array([[-1.0]]), [False])


def test_r_sd_is_na_at_one_value():
    assert model.r_sd([3.0]) is None and model.r_sd([1.0, 3.0]) == 2.0 ** 0.5


def small_tree(columns_by_cluster, names=("a", "b", "c")):
    """Clusters of G = 5 positions flipped F, T, F, F, T; columns_by_cluster: cluster number -> [S] columns of 5 cells as the statistics see them."""
    tree = {}
    for c, cols in columns_by_cluster.items():
        data = np.array(cols, dtype=np.float64).T
        rows = np.where(np.array(FLIP)[:, None], 100.0 - data, data)
        tree["sp_%d.pos.freq" % c] = cases.freq_text(["k:-:%d:A" % p for p in range(5)], rows)
        tree["sp_%d_hap_positions.tab" % c] = cases.hap_text(["k:-:%d:T>A:." % p for p in range(5)], FLIP)
    return tree, cases.all_samples_text(names)


def test_keep_rule_is_the_codes_not_the_comments():
    one, none, full = [NAN, NAN, 100, NAN, NAN], [NAN] * 5, [100, 100, 100, 0, 100]
    # cluster 1: a column with one called cell of five is kept at 0.2 (1 >= 0.2 * 5), one with none is not; two kept columns: used
    tree, samples = small_tree({1: [one, none, full]})
    files, info = model.profile_files("sp", samples, tree)
    assert info["status"] == model.OK and info["n_usable"] == 1 and info["n_full"] == 2
    assert files["sp_extended_clustering_abundanceSummaryStats.tsv"] == model.SUMMARY_HEADER + "a\t1\t100\t100\tNA\t1\t1\t0\t1\t4\nc\t1\t80\t100\t44.7213595499958\t0.8\t0.8\t1\t4\t0\n"
    # exactly one kept column: the cluster is skipped ("Insufficient data"); none: skipped too ("No data")
    tree, samples = small_tree({1: [one, none, full], 2: [none, none, full], 3: [none, none, none]})
    files, info = model.profile_files("sp", samples, tree)
    assert info["n_files"] == 3 and info["n_usable"] == 1 and "\t2\t" not in files["sp_extended_clustering_abundanceSummaryStats.tsv"]
    tree, samples = small_tree({1: [none, none, full], 2: [none, none, none]})
    files, info = model.profile_files("sp", samples, tree)
    assert info["status"] == model.NONE_USABLE and files == {"sp_extended_clustering_stat.txt": "Species sp: 0/2 clusters had usable placing data.\n"}
    for bad in (0.0, 1.5, -0.2):
        with pytest.raises(model.DomainError):
            model.profile_files("sp", samples, tree, max_prop_uncalled=bad)


def test_ids_with_and_without_annotation():
    assert model.freq_id("515620.PRJNA29073.CP001104:-:1219674:A") == "515620.PRJNA29073.CP001104:1219674:A"
    assert model.hap_id("515620.PRJNA29073.CP001104:-:1219674:T>A:.") == "515620.PRJNA29073.CP001104:1219674:A"
    assert model.freq_id("c1:geneX:12:C") == "c1:12:C" and model.hap_id("c1:geneX:12:G>C:N[AAT-ACT]") == "c1:12:C"
    assert model.hap_id("c1:-:12:C:.") == "c1:12:C"                     # a table whose labels carry the allele alone
    with pytest.raises(model.FormatError):
        model.freq_id("c1:12:C")


def test_cluster_files_in_byte_order_and_their_numbers():
    names = ["sp_2.pos.freq", "sp_10.pos.freq", "sp_1.pos.freq", "sp_1.pos", "spx_1.pos.freq", "sp_1_hap_positions.tab", "other_sp_1.pos.freq"]
    assert model.cluster_files("sp", names) == ["sp_1.pos.freq", "sp_10.pos.freq", "sp_2.pos.freq"]
    assert model.cluster_number("ref_mOTU_v2_2227_10.pos.freq") == ("ref_mOTU_v2_2227_10", 10)
    with pytest.raises(model.FormatError):
        model.cluster_number("sp_a.pos.freq")


def test_stat_lines_verbatim():
    assert model.stat_none_usable("sp", 3) == "Species sp: 0/3 clusters had usable placing data.\n"
    assert model.stat_incoherent("sp", 37, 1, 2) == ("Species sp: 3 out of 37 samples rejected due to incoherent subpecies assignment. Number of samples where summed abundance "
                                                     "of clusters was < 80%: 1. Number of samples where summed abundance of clusters was > 120%:2\n")
    assert model.stat_bad("sp", 1, 34) == ("Species sp: 1 out of 34 samples rejected due to extreme mismatch between median abundance of genotyping SNVs (>30%) and "
                                           "prevalence of genotyping SNVs (<75%).\n")
    assert model.profile_files("sp", "a\nb\n", {})[0] == {"sp_extended_clustering_stat.txt": "Species sp: 0/0 clusters had usable placing data.\n"}


def test_clustering_table():
    text = model.clustering_table(["none", "one", "two", "edge"], [[50.0, 50.0, 0.0], [0.0, 95.5, 4.0], [81.0, 0.0, 90.0], [80.0, 20.0, 0.0]])
    assert text == "clust\nnone\tNA\none\t2\ntwo\tNA\nedge\tNA\n"       # strictly above 80; the value is the column's position


def test_the_planted_project_holds_every_case():
    tree, samples, truth = cases.planted_project()
    files, info = model.profile_files("sp", samples, tree)
    names = model.sample_names(samples)
    assert names[0] == "s0001.bam" and len(names) == 40
    assert info == dict(status=model.OK, n_files=3, n_usable=3, n_full=39, n_filtered=36, n_incoherent=2, n_bad=1, n_assigned=35)
    assert files["sp_extended_clustering_stat.txt"] == model.stat_incoherent("sp", 39, 1, 1) + model.stat_bad("sp", 1, 37)
    summary = files["sp_extended_clustering_abundanceSummaryStats.tsv"].split("\n")
    assert len(summary) == 1 + 3 * 39 + 1 and not any(ln.startswith(names[cases.LOW_COVERAGE] + "\t") for ln in summary)
    assert any(ln.endswith("\t%d" % (45 - n)) for n in range(46) for ln in summary if "\t2\t" in ln)
    unfiltered = files["sp_extended_clustering_wFreq_unfiltered.tab"].split("\n")
    assert unfiltered[0] == "1\t2\t3" and len(unfiltered) == 1 + 39 + 1
    clust = dict(ln.split("\t") for ln in files["sp_extended_clustering.tab"].split("\n")[1:] if ln)
    for s in (cases.LOW_COVERAGE, cases.SUM_HIGH, cases.SUM_LOW, cases.BAD):
        assert names[s] not in clust
    assert clust.pop(names[cases.MIXED]) == "NA"
    assert all(clust[names[s]] == str(truth[s]) for s in range(40) if names[s] in clust) and len(clust) == 35


def test_where_the_reference_breaks():
    full = [100, 100, 100, 0, 100]
    tree, samples = small_tree({2: [full, full, full], 3: [full, full, full]})
    with pytest.raises(model.DomainError) as err:
        model.profile_files("sp", samples, tree)
    assert "cluster 1" in str(err.value) and list(err.value.files) == ["sp_extended_clustering_abundanceSummaryStats.tsv"]
    none = [NAN] * 5
    tree, samples = small_tree({1: [full, full, none, none], 2: [none, none, full, full]}, names="abcd")
    with pytest.raises(model.DomainError) as err:
        model.profile_files("sp", samples, tree)
    assert "no sample" in str(err.value)


# ---------------------------------------------------------------------------------------------- the abundance stage (host only: the library runs here)
WFREQ = "1\t2\ns1.bam\t100\t0\ns2.bam\t12.5\t87.5\ns3.bam\t33.3333333333333\t60\n"
ABUND = "# a species abundance table\n\ts2.bam\ts9.bam\ts1.bam\ts3.bam\nother\t1\t1\t1\t1\nsp\t0.5\t7\t0.25\t0.3\n"


def run_abundance(tmp_path, wfreq, abund, suffix=None):
    os.makedirs(str(tmp_path), exist_ok=True)
    open(str(tmp_path / "sp_extended_clustering_wFreq.tab"), "w").write(wfreq)
    open(str(tmp_path / "abund.tsv"), "w").write(abund)
    before = set(os.listdir(str(tmp_path)))
    counts = subpopr.subpop_abundance_files("sp", str(tmp_path), str(tmp_path / "abund.tsv"), suffix)
    files, want = model.abundance_files("sp", wfreq, abund, suffix)
    assert counts == want
    assert sorted(set(os.listdir(str(tmp_path))) - before) == sorted(files)
    for f in files:
        assert open(str(tmp_path / f)).read() == files[f], f
    return files


def test_abundance_exact_text(tmp_path):
    files = run_abundance(tmp_path, WFREQ, ABUND)
    assert files["sp_allClust_relativeAbund.tab"] == "X1\tX2\ns2.bam\t0.0625\t0.4375\ns1.bam\t0.25\t0\ns3.bam\t0.0999999999999999\t0.18\n"
    assert files["sp_clust_2_hap_coverage_extended_normed.tab"] == "X2\ns2.bam\t0.4375\ns1.bam\t0\ns3.bam\t0.18\n"
    assert sorted(files) == ["sp_allClust_relativeAbund.tab", "sp_clust_1_hap_coverage_extended_normed.tab", "sp_clust_2_hap_coverage_extended_normed.tab"]


def test_abundance_suffix_retry(tmp_path):
    abund = ABUND.replace(".bam", "")
    files = run_abundance(tmp_path / "a", WFREQ, abund, ".bam")
    assert files["sp_allClust_relativeAbund.tab"].startswith("X1\tX2\ns2.bam\t0.0625\t")
    with pytest.raises(MsnvError) as err:                               # no suffix given: no retry
        subpopr.subpop_abundance_files("sp", str(tmp_path / "a"), str(tmp_path / "a" / "abund.tsv"))
    assert err.value.code == EDOMAIN and "No overlapping sample IDs between clustering and apecies abundance profiles." in str(err.value)
    assert "Example clustering IDs: s1.bam, s2.bam, s3.bam. Example species profile IDs:s9, s1, s3" in str(err.value)
    with pytest.raises(model.DomainError) as merr:
        model.abundance_files("sp", WFREQ, abund)
    assert str(merr.value) in str(err.value)


def test_abundance_refusals(tmp_path):
    for wfreq, abund, text in ((WFREQ, ABUND.replace("\nsp\t", "\nsq\t"), "Species not found in the species abundance profile. Species: sp"),
                               (WFREQ, ABUND + "sp\t1\t1\t1\t1\n", "More than one species in the abundance profile matched for species named: sp"),
                               ("1\t2\n", ABUND, "Species does not have cluster frequencies. Species: sp")):
        with pytest.raises(model.DomainError) as merr:
            model.abundance_files("sp", wfreq, abund)
        assert str(merr.value) == text
        open(str(tmp_path / "sp_extended_clustering_wFreq.tab"), "w").write(wfreq)
        open(str(tmp_path / "abund.tsv"), "w").write(abund)
        with pytest.raises(MsnvError) as err:
            subpopr.subpop_abundance_files("sp", str(tmp_path), str(tmp_path / "abund.tsv"))
        assert err.value.code == EDOMAIN and text in str(err.value)
    assert not [f for f in os.listdir(str(tmp_path)) if "relativeAbund" in f or "normed" in f]


# ---------------------------------------------------------------------------------------------- the launchers
def launch(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), capture_output=True, text=True)


def test_profile_launcher(tmp_path):
    out, meta = tmp_path / "out", tmp_path / "metasnv"
    os.makedirs(str(out)), os.makedirs(str(meta))
    r = launch("profileSubpops.py", "sp", str(meta), str(out))
    assert r.returncode == 0 and r.stdout.startswith("No distinctive genotyping positions for species sp, perhaps the cutoff was bad. See ")
    assert "(Required file does not exist: " + str(out / "sp_hap_freq_median.tab") + ")" in r.stdout
    open(str(out / "sp_hap_freq_median.tab"), "w").write("\ti\n")
    r = launch("profileSubpops.py", "sp", str(meta), str(out))
    assert r.returncode != 0 and "File with paths to samples does not exist." in r.stderr and str(meta / "all_samples") in r.stderr
    open(str(meta / "all_samples"), "w").write("/x/a.bam\n/x/b.bam\n")
    r = launch("profileSubpops.py", "sp", str(meta), str(out))
    if core.device_count() < 1:
        assert r.returncode != 0 and "no CPU fallback" in r.stderr and not os.path.exists(str(out / "sp_extended_clustering_stat.txt"))
    else:                                                               # with a device it runs, and finds no cluster file
        assert r.returncode == 0 and open(str(out / "sp_extended_clustering_stat.txt")).read() == model.stat_none_usable("sp", 0)


def test_abundance_launcher(tmp_path):
    r = launch("writeSubpopAbund.py", "sp", str(tmp_path), str(tmp_path / "abund.tsv"))
    assert r.returncode == 0 and r.stdout.startswith("Species sp does not have cluster frequencies. File does not exist: ")
    open(str(tmp_path / "sp_extended_clustering_wFreq.tab"), "w").write(WFREQ)
    r = launch("writeSubpopAbund.py", "sp", str(tmp_path), str(tmp_path / "abund.tsv"))
    assert r.returncode != 0 and "Required species abundance file not found: " + str(tmp_path / "abund.tsv") in r.stderr
    open(str(tmp_path / "abund.tsv"), "w").write(ABUND.replace(".bam", ""))
    r = launch("writeSubpopAbund.py", "sp", str(tmp_path), str(tmp_path / "abund.tsv"), "--sample-suffix", ".bam")
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "sp_allClust_relativeAbund.tab")).read() == model.abundance_files("sp", WFREQ, ABUND)[0]["sp_allClust_relativeAbund.tab"]
