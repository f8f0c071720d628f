"""metaSNV_subpopr.py on the device (metasnv_amd/subpopr_run.py) and the cluster stage's -x / -y (msnv_cluster_file_ex): the driver's files against the
files the stage functions write when they are called one by one, its summaries against texts derived from those, and the stage's sample filter
against numpy on a table whose cells stand on the edges of the 10/90 and 20/80 bands.  Every comparison is of bytes.  24 samples a species,
--stability-iters 2 --boot 5 --minNumSamples 12 --seed 7, and a prediction-strength cut of 0.5 (subpoprruncases.PS_CUT says why)."""
import ctypes as C
import glob
import os
import re

import pytest

import pamcases
import subpoprruncases as cases
from metasnv_amd import _lib, core, subpopr, subpopr_run as run
from metasnv_amd._lib import MsnvError, EINVAL, CLUSTER_OK

pytestmark = pytest.mark.gpu
OUT_NAME = os.path.join("params.hr10.hs80.ps50.gs80", "proj")
INSUFFICIENT_303 = "Insufficient number of samples in metaSNV filtered SNV results (8 samples)"


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------- 1. the cluster stage's options
@pytest.fixture(scope="module")
def edge_case(tmp_path_factory):
    root = tmp_path_factory.mktemp("edge")
    names, dist, order, table = cases.band_edge_table()
    dist_path, freq_path = str(root / "sp.filtered.mann.dist"), str(root / "sp.filtered.freq")
    pamcases.write_dist(dist_path, names, dist)
    pamcases.write_freq(freq_path, [names[i] for i in order], table[:, order])
    return root, names, order, table, dist_path, freq_path


def run_filter(ctx, edge_case, tag, **kw):
    root, _, _, _, dist_path, freq_path = edge_case
    out = str(root / tag)
    res = subpopr.cluster_file(ctx, dist_path, out, freq_path=freq_path, **dict(cases.STAGE_OPTS, **kw))
    return res, cases.read_tree(out)


def composition(tree):
    (name,) = [k for k in tree if k.endswith("_freq_composition.tab")]
    return tree[name]


def used_samples(tree):
    (name,) = [k for k in tree if k.endswith("_mann_distMatrixUsedForClustMedoidDefns.txt") and not k.startswith("clustMedoidDefnFailed")]
    return tree[name].decode().splitlines()[0].split("\t")


def test_null_filter_and_the_defaults_write_the_files_of_msnv_cluster_file(ctx, edge_case):
    root, _, _, _, dist_path, freq_path = edge_case
    o = _lib.ClusterOpts()
    _lib.lib.msnv_cluster_opts_default(C.byref(o))
    o.seed, o.ps_cut, o.stability_iters = cases.STAGE_OPTS["seed"], cases.STAGE_OPTS["ps_cut"], cases.STAGE_OPTS["stability_iters"]
    res, ms = (C.c_int64 * 8)(), C.c_double()
    _lib.check(_lib.lib.msnv_cluster_file(ctx._h, dist_path.encode(), freq_path.encode(), b"sp", str(root / "plain").encode(), C.byref(o), res, C.byref(ms)))
    plain = cases.read_tree(str(root / "plain"))
    assert res[0] == CLUSTER_OK and "sp_mann_clustering.tab" in plain and "sp_freq_composition.tab" in plain
    res_null, null = run_filter(ctx, edge_case, "null")
    res_dflt, dflt = run_filter(ctx, edge_case, "defaults", max_prop_reads_non_homog=0.1, min_prop_homog_snv=0.8)
    assert null == plain and dflt == plain
    assert [res_null[k] for k in ("status", "n_clusters", "n_samples", "n_outliers")] == [res[0], res[1], res[2], res[3]] == [res_dflt[k] for k in ("status", "n_clusters", "n_samples", "n_outliers")]
    f = _lib.ClusterFilter()
    _lib.lib.msnv_cluster_filter_default(C.byref(f))
    assert (f.max_prop_reads_non_homog, f.min_prop_homog_snv) == (0.1, 0.8)
    assert plain["sp_freq_composition.tab"].decode().splitlines()[0] == "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95"


def test_fix_read_threshold_selects_by_its_own_strict_band(ctx, edge_case):
    _, names, order, table, _, _ = edge_case
    _, everybody = run_filter(ctx, edge_case, "y0", min_prop_homog_snv=0.0)
    after_outliers = used_samples(everybody)                              # -y 0: no filter, every sample left after outlier removal, in matrix order
    root, _, _, _, dist_path, _ = edge_case
    subpopr.cluster_file(ctx, dist_path, str(root / "nofreq"), **cases.STAGE_OPTS)
    assert after_outliers == used_samples(cases.read_tree(str(root / "nofreq"))) and set(after_outliers) <= set(names) and len(after_outliers) >= 19
    for tag, x, y in (("x01", 0.1, 0.8), ("x02", 0.2, 0.8), ("x02y09", 0.2, 0.9)):
        res, tree = run_filter(ctx, edge_case, tag, max_prop_reads_non_homog=x, min_prop_homog_snv=y)
        want = [names[s] for s in order if names[s] in after_outliers and cases.strict_proportion(table[:, s], x) >= y]      # the frequency table's order
        assert used_samples(tree) == want and res["n_samples"] == len(want), tag
        assert composition(tree) == composition(everybody)            # three fixed columns whatever -x is
    kept = lambda x, y: {s for s in cases.EDGE_SAMPLES if cases.strict_proportion(table[:, s], x) >= y}
    assert kept(0.1, 0.8) == {2, 7, 17} and kept(0.2, 0.8) == {2, 5, 7, 13, 17} and kept(0.2, 0.9) == {2, 5, 13}      # the table does tell the bands apart


def test_fix_read_threshold_is_folded_at_one_half(ctx, edge_case):
    _, at01 = run_filter(ctx, edge_case, "fold01", max_prop_reads_non_homog=0.1)
    _, at09 = run_filter(ctx, edge_case, "fold09", max_prop_reads_non_homog=0.9)
    assert at09 == at01 and (1.0 - 0.9) * 100.0 != 10.0                   # another band in double, the same cells outside it


@pytest.mark.parametrize("kw", [dict(max_prop_reads_non_homog=1.5), dict(max_prop_reads_non_homog=-0.1), dict(min_prop_homog_snv=1.5), dict(min_prop_homog_snv=float("nan")),
                                dict(max_prop_reads_non_homog=float("nan"))])
def test_filter_outside_0_to_1_is_refused_before_anything_is_read(ctx, edge_case, kw):
    root = edge_case[0]
    with pytest.raises(MsnvError) as e:
        subpopr.cluster_file(ctx, str(root / "no_such_file.dist"), str(root / "refused"), freq_path=str(root / "no_such_file.freq"), **kw)
    assert e.value.code == EINVAL
    with pytest.raises(MsnvError) as e:
        run_filter(ctx, edge_case, "refused", **kw)
    assert e.value.code == EINVAL and not os.path.exists(str(root / "refused"))


# ---------------------------------------------------------------------------------------------- 2. one project of five species
@pytest.fixture(scope="module")
def project(tmp_path_factory):
    root = tmp_path_factory.mktemp("five")
    proj = str(root / "proj")
    abund, genes = cases.five_species_project(proj)
    summary = run.main(["-i", proj, "-o", str(root / "results"), "-a", abund, "-m", "FALSE", "-g", genes] + cases.DRIVER_OPTS)
    return root, proj, abund, genes, os.path.join(str(root / "results"), OUT_NAME), summary


def test_species_seen_and_their_results(project):
    root, proj, _, _, out, summary = project
    assert summary["out_dir"] == out and list(summary["species"]) == ["101", "202", "303", "404"]
    assert summary["species"]["101"] == "nClusters = 2" and summary["species"]["202"] == "nClusters = 1" and summary["species"]["404"] == "nClusters = 2"
    assert summary["species"]["303"] == INSUFFICIENT_303
    assert summary["ms_kernel"] > 0 and summary["wall_s"] > 0
    log = open(os.path.join(out, "log.txt")).read()
    assert re.search(r"Warning: Species indicated in .* are not identical.*Species not found in both locations: 505", log)
    assert not [f for dp, _, files in os.walk(out) for f in files if f.startswith("505") or f.startswith("303")]
    tree = cases.read_tree(out)
    assert "noClustering/202_mann_clustering.tab" in tree and "noClustering/202_mann_pcoa_eig.tab" in tree and "noClustering/202_mann_heatmap_all.tab" in tree
    assert "202_mann_clustering.tab" not in tree and "202_hap_out.txt" not in tree
    assert '"202","No clusters","NA","NA"' in tree["summary_clusteringExtension.csv"].decode().splitlines()


def test_the_drivers_files_of_a_species_are_those_of_its_stages_called_one_by_one(ctx, project):
    root, proj, abund, genes, out, _ = project
    solo = str(root / "solo")
    dist_path, freq_path = os.path.join(proj, "distances", "101.filtered.mann.dist"), os.path.join(proj, "filtered", "pop", "101.filtered.freq")
    subpopr.snv_freq_file(ctx, freq_path, solo, species="101", max_prop_reads_non_homog=0.1, min_prop_homog_snv=0.8)
    res = subpopr.cluster_file(ctx, dist_path, solo, species="101", freq_path=freq_path, max_prop_reads_non_homog=0.1, min_prop_homog_snv=0.8, **cases.STAGE_OPTS)
    assert res["status"] == CLUSTER_OK and res["n_clusters"] == 2
    subpopr.membership_stability_file(ctx, os.path.join(solo, "101_mann_distMatrixUsedForClustMedoidDefns.txt"), "101", subpopr.clusters_from_ps_values(solo, "101", cases.PS_CUT),
                                      solo, clus_num_stability_path=os.path.join(solo, "101_mann_clusNumStability.tab"), seed=7, boot_iters=5)
    subpopr.pcoa_file(ctx, dist_path, solo, species="101")
    subpopr.genotype_file(ctx, os.path.join(solo, "101_mann_clustering.tab"), freq_path, solo, species="101", uniq_threshold=0.8)
    subpopr.heatmap_file(ctx, dist_path, solo, species="101")
    haps = sorted(glob.glob(os.path.join(solo, "*hap_positions.tab")))
    assert len(haps) == 2
    subpopr.genotyping_subset(haps, [os.path.join(proj, "snpCaller", "called_SNPs.best_split_1")], solo)
    for pos in sorted(glob.glob(os.path.join(solo, "*.pos"))):
        subpopr.snv_allele_freq(ctx, pos, 5)
    subpopr.subpop_profile_files(ctx, "101", solo, os.path.join(proj, "all_samples"))
    subpopr.subpop_abundance_files("101", solo, abund)
    subpopr.gene_corr_files(ctx, os.path.join(solo, "101_allClust_relativeAbund.tab"), genes, os.path.join(solo, "101_corrGenes"))
    want, got = cases.read_tree(solo), cases.read_tree(out)
    assert len(want) >= 25 and {"101_1.pos.freq", "101_extended_clustering_wFreq.tab", "101_corrGenes-spearman.tsv", "101_mann_pcoa_proj.tab", "101_mann_stabilityAssessment.tab",
                                "snvFreqPlots/101_snvFreq_fixed.tab", "101_mann_heatmap_discovery.tab", "101_clust_2_hap_coverage_extended_normed.tab"} <= set(want)
    for rel in want:
        assert got[rel] == want[rel], rel
    assert sorted(k for k in got if re.match(r"(snvFreqPlots/)?101[_.]", k)) == sorted(want)      # and the driver writes no other file for the species


def test_na_cells_and_a_missing_column_equal_a_table_cleaned_by_hand(project):
    root, _, _, _, out, summary = project
    proj = str(root / "by_hand" / "proj")
    abund, genes = cases.five_species_project(proj, by_hand=True)
    by_hand = run.main(["-i", proj, "-o", str(root / "by_hand" / "results"), "-a", abund, "-m", "FALSE", "-g", genes] + cases.DRIVER_OPTS)
    assert by_hand["species"] == {"404": summary["species"]["404"]}
    want = {k: v for k, v in cases.read_tree(by_hand["out_dir"]).items() if re.match(r"(snvFreqPlots/)?404[_.]", k)}
    got = {k: v for k, v in cases.read_tree(out).items() if re.match(r"(snvFreqPlots/)?404[_.]", k)}
    assert len(want) >= 25 and got == want
    assert not os.path.exists(os.path.join(by_hand["out_dir"], "inputs"))
    cleaned = open(os.path.join(out, "inputs", "404.filtered.mann.dist")).read().splitlines()
    assert cleaned == open(os.path.join(proj, "distances", "404.filtered.mann.dist")).read().splitlines() and os.listdir(os.path.join(out, "inputs")) == ["404.filtered.mann.dist"]
    assert cases.EXTRA not in cleaned[0] and len(cleaned) == cases.N


def table_rows(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()[1:]]


def test_summaries_follow_from_the_stage_files(project):
    _, _, _, _, out, summary = project
    text = lambda name: open(os.path.join(out, name)).read()
    assert text("log_clusteringSummaryPerSpecies.txt") == '"result" "species"\n' + "".join('"%s" "%s"\n' % (summary["species"][sp], sp) for sp in ("101", "202", "303", "404"))
    ext = {}
    for sp in ("101", "404"):
        clust = [r[1] for r in table_rows(os.path.join(out, sp + "_extended_clustering.tab"))]
        sizes = "-".join(str(clust.count(c)) for c in ("1", "2"))
        snvs = "-".join(str(len(table_rows(os.path.join(out, "%s_%d_hap_positions.tab" % (sp, c))))) for c in (1, 2))
        assert sizes == "12-12" and snvs == "16-16"                       # the planted halves; each of the 16 planted positions tells both apart
        ext[sp] = '"%s","Succeeded","%s","%s"' % (sp, sizes, snvs)
    ext["202"] = '"202","No clusters","NA","NA"'
    assert text("summary_clusteringExtension.csv") == '"speciesID","ClusterGenotyping","GenotypedClusterSizes","nSNVs"\n' + "".join(ext[sp] + "\n" for sp in ("101", "202", "404"))
    rows = []
    for f in sorted(os.listdir(out)):
        if f.endswith("_hap_coverage_extended_normed.tab"):
            rows += [(r[0], f.split("_")[0], f.split("_")[2], r[1]) for r in table_rows(os.path.join(out, f))]
    assert len(rows) == 4 * cases.N
    assert text("subpopAbunds.tsv") == "sampleName\tspecies\tsubpop\tabundance\n" + "".join("\t".join(r) + "\n" for r in sorted(rows, key=lambda r: r[0]))
    clustering = text("summary_clustering.csv").splitlines()
    assert [ln.split(",")[1] for ln in clustering[1:]] == ['"101"', '"404"', '"202"']      # the order of the files' paths
    genes = dict((ln.split(",")[0], ln.split(",", 1)[1]) for ln in text("summary_geneFamilyCorrAssoc.csv").splitlines())
    assert genes['"101"'].startswith('"Correlations calculated",') and genes['"202"'] == '"No correlation results",FALSE,NA'
    by_species = {ln.split(",")[1]: ln.split(",", 1)[1] for ln in clustering}
    assert text("summary_allResults.csv") == "".join(
        by_species[key] + "," + tail.split(",", 1)[1] + "," + genes[key] + "\n"
        for key, tail in [('"speciesID"', '"speciesID","ClusterGenotyping","GenotypedClusterSizes","nSNVs"')] + [('"%s"' % sp, ext[sp]) for sp in ("101", "202", "404")])
    stats = text("subpopFreqSumsStats.tsv").splitlines()
    assert stats[0].split("\t")[:3] == ["species", "nClus", "nSamples"] and sorted(ln.split("\t")[0] for ln in stats[1:]) == ["101", "404"]


# ---------------------------------------------------------------------------------------------- 3. further runs
def test_existing_clustering_and_genotyping_are_left_alone(project):
    root, proj, abund, genes, out, _ = project
    # what the clustering, its ratings, the ordination, the genotyping and the raw-SNV subset wrote; the heatmap orders are written again (same bytes)
    kept = re.compile(r"_mann_(PS_values|distMatrixUsed|clustering|clusNumStability|clusMembStability|stabilityAssessment|pcoa_)|_freq_composition|_snvFreq_|\.pos(\.freq)?$"
                      r"|_hap_(positions|out|freq_)")
    frozen = lambda: {k: (v, os.stat(os.path.join(out, k)).st_mtime_ns) for k, v in cases.read_tree(out).items() if kept.search(k)}
    profiles = lambda: {k: v for k, v in cases.read_tree(out).items() if "_extended_clustering" in k and not k.endswith("_stat.txt")}      # _stat.txt is appended to
    rest = lambda: {k: v for k, v in cases.read_tree(out).items() if not k.endswith(("_stat.txt", "log.txt"))}
    before, profiles_before, rest_before = frozen(), profiles(), rest()
    for k in profiles_before:
        os.remove(os.path.join(out, k))
    assert len(before) >= 50 and len(profiles_before) >= 8
    again = run.main(["-i", proj, "-o", str(root / "results"), "-a", abund, "-m", "FALSE", "-g", genes, "--useExistingClustering", "TRUE", "--useExistingGenotyping", "TRUE"]
                     + cases.DRIVER_OPTS)
    assert again["out_dir"] == out and again["species"] == {}
    assert frozen() == before and profiles() == profiles_before and rest() == rest_before


def test_only_subspecies_detection_stops_after_the_clustering_summary(project):
    root, proj, _, _, _, _ = project
    summary = run.main(["-i", proj, "-o", str(root / "q"), "-q", "TRUE"] + cases.DRIVER_OPTS)
    out = summary["out_dir"]
    assert summary["species"]["101"] == "nClusters = 2" and os.path.exists(os.path.join(out, "101_hap_out.txt"))
    lines = open(os.path.join(out, "summary_allResults.csv")).read().splitlines()
    assert lines[0].startswith('"speciesID","speciesName",') and [ln.split(",")[0] for ln in lines[1:]] == ['"101"', '"202"', '"404"']
    assert not glob.glob(os.path.join(out, "*.pos")) and not os.path.exists(os.path.join(out, "summary_clusteringExtension.csv"))
    assert "Subpopr stopped due to 'onlyDoSubspeciesDetection' flag being true" in open(os.path.join(out, "log.txt")).read()


def test_a_species_that_fails_is_recorded_and_the_others_finish(tmp_path):
    proj = str(tmp_path / "proj")
    cases.two_species_project(proj)
    summary = run.main(["-i", proj, "-o", str(tmp_path / "results"), "-q", "TRUE"] + cases.DRIVER_OPTS)
    assert summary["species"]["101"] == "nClusters = 2"
    assert summary["species"]["909"].startswith("ERROR:")
    assert "The max value in your SNV frequency file is > 1. Values are expected to be -1 or within [0 to 1]. Are you using an old version of metaSNV?" in summary["species"]["909"]
    out = summary["out_dir"]
    assert os.path.exists(os.path.join(out, "101_hap_out.txt")) and not [f for f in os.listdir(out) if f.startswith("909")]
    assert '" "909"\n' in open(os.path.join(out, "log_clusteringSummaryPerSpecies.txt")).read()
