"""tests/membstabmodel.py, the numpy restatement the GPU membership-stability tests compare with (tests/test_gpu_membstab.py), pinned on its own:
hand-worked Jaccard pairs, the score rule on small tables, the exact text of both files and of summary_clustering.csv, and both launchers as
far as they go without a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import membstabmodel as model
import pamcases as cases
from metasnv_amd import subpopr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def line(xs):
    x = np.asarray(xs, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


# ---------------------------------------------------------------------------------- the Jaccard pairs
def test_worked_case_both_reclusterings():
    # members 0..5, A = {0, 1, 2}, B = {3, 4, 5}; the subset [0, 1, 3, 4] holds two of each
    orig = [1, 1, 2, 2]
    # re-clustered as {0, 1}, {3, 4}: A meets cluster 1 in 2 of 2 + 2 - 2, B likewise
    assert model.best_pairs(orig, [1, 1, 2, 2], 2) == [(2, 2), (2, 2)]
    # re-clustered as {0}, {1, 3, 4}: A: 1 / (2 + 1 - 1) = 1/2 against 1 / (2 + 3 - 1) = 1/4; B: 0 / 3 against 2 / (2 + 3 - 2)
    assert model.best_pairs(orig, [1, 2, 2, 2], 2) == [(1, 2), (2, 3)]


def test_equal_fractions_keep_the_first_and_empty_new_clusters_are_passed_over():
    # A = 4 entries, new clusters {a, a} {a, a}: 2/4 both times -> the first; pairs (2, 4)
    assert model.best_pairs([1, 1, 1, 1], [1, 1, 2, 2], 2) == [(2, 4), (0, 2)]
    # new cluster 1 has no entry (its medoid is a duplicate): it is never the match, even for an original cluster that is absent too
    assert model.best_pairs([2, 2, 2], [2, 2, 2], 2) == [(0, 3), (3, 3)]


def test_the_worked_case_through_pam():
    # two groups on a line; the subset [0, 1, 3, 4] re-clusters as {0, 1}, {3, 4}
    d = line([0, 1, 2, 10, 11, 12])
    clus, med, pairs = model.cluster_boot(d, list(range(6)), 2, [[0, 1, 3, 4], [4, 3, 1, 0]])
    assert clus.tolist() == [1, 1, 1, 2, 2, 2] and med.tolist() == [1, 4]
    assert pairs.tolist() == [[[2, 2], [2, 2]], [[2, 2], [2, 2]]]


def test_a_set_that_misses_an_original_cluster():
    d = line([0, 1, 2, 10, 11, 12, 30, 31, 32])
    clus, _, pairs = model.cluster_boot(d, list(range(9)), 3, [[0, 1, 2, 3, 4, 5]])
    assert clus.tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    inter, union = pairs[0, 2]
    assert inter == 0 and union > 0 and inter / union == 0.0      # cluster 3 has no entry in the subset
    assert pairs[0, :2, 0].tolist() != [0, 0]


def test_far_apart_planted_groups_are_always_recovered():
    d = cases.planted_dist(40, 2, 3)
    sizes, rows, n_sets = model.memb_rows(d, 2, seed=5, boot_iters=4)
    assert sizes == [20, 20] and n_sets == 4 * len(rows) and [round(p, 1) for p, _ in rows] == [0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    for _, per in rows:
        assert per == [(1.0, INF), (1.0, INF)]
    assert [model.memb_score(rows, j) for j in range(2)] == [3, 3]


# ---------------------------------------------------------------------------------- the score rule
def table(at90, at70=None, at100=(1.0, INF)):
    rows = [(0.7000000000000001, [at70])] if at70 is not None else []
    return rows + [(0.9, [at90]), (1.0, [at100])]                # (prop, [(jaccard, recover)])


def test_score_rule():
    assert model.memb_score(table((0.85, 0.7), (0.95, 0.6)), 0) == 1                  # Low: recover fails both times
    assert model.memb_score(table((0.85, 0.9), (0.85, 0.95)), 0) == 2                 # Medium by the 0.9 term
    assert model.memb_score(table((0.7, 0.9), (0.95, 0.95)), 0) == 2                  # Medium by the 0.7 term alone: the terms add independently
    assert model.memb_score(table((0.85, INF), (0.95, INF)), 0) == 3                  # High; Inf > 0.9
    assert model.memb_score(table((0.8, 0.9), (0.9, 0.95)), 0) == 1                   # the comparisons are strict
    assert model.memb_score(table((0.85, NAN), (0.95, 0.95)), 0) == 0                 # TRUE & NA = NA
    assert model.memb_score(table((0.5, NAN), (0.95, 0.95)), 0) == 2                  # FALSE & NA = FALSE: the term counts as 0
    assert model.memb_score(table((0.85, 0.9)), 0) == 0                               # no 0.7 row (n < 15): NA
    assert model.memb_score(table(None, (0.95, 0.95)), 0) == 0                        # a row of NA (subset size <= k)
    assert model.and3(False, None) is False and model.and3(None, True) is None and model.and3(True, True) is True


# ---------------------------------------------------------------------------------- the text
MEMB = ("clusterID\tnSamplesInCluster\tsubsampleProp\tclusterStabilityJaccardMean\tclusterStabilityPropRecover\n"
        "1\t7\t0.9\t0.875\tInf\n2\t5\t0.9\t0.5\t0\n1\t7\t1\t1\tInf\n2\t5\t1\tNA\tNA\n")


def test_text_of_both_files():
    rows = [(0.9, [(0.875, INF), (0.5, 0.0)]), (1.0, [(1.0, INF), None])]
    assert model.memb_text([7, 5], rows) == MEMB
    assert model.memb_text([3], [(0.30000000000000004, [(1.0 / 3.0, NAN)])]).splitlines()[1] == "1\t3\t0.3\t0.333333333333333\tNaN"
    assert model.assessment_text(3, [3, 0]) == "name\tscore\nnumClusters\tHigh\nclust1\tHigh\nclust2\tNA\n"
    assert model.assessment_text(0, [1]) == "name\tscore\nnumClusters\tNA\nclust1\tLow\n"


def project():
    """Three species: one with clusters, one in noClustering/, one without stability files."""
    used = lambda n: "\t".join("s%d" % i for i in range(n)) + "\n" + "".join("s%d\t" % i + "\t".join(["0"] * n) + "\n" for i in range(n))
    return {
        "spB_mann_clustering.tab": "clust\ns0\t1\n",
        "spB_mann_distMatrixUsedForClustMedoidDefns.txt": used(12),
        "spB_mann_PS_values.tab": "x\n1\t1\n2\t0.912345\n3\t0.5\n",
        "spB_mann_clusMembStability.tab": MEMB,
        "spB_mann_stabilityAssessment.tab": "name\tscore\nnumClusters\tMedium\nclust1\tHigh\nclust2\tNA\n",
        "noClustering/spA_mann_clustering.tab": "clust\ns0\t1\n",
        "noClustering/spA_mann_distMatrixUsedForClustMedoidDefns.txt": used(10),
        "noClustering/spA_mann_PS_values.tab": "x\n1\t1\n2\t0.25\n",
        "noClustering/spA_mann_clusMembStability.tab": MEMB.split("\n")[0] + "\n1\t10\t1\t1\tInf\n",
        "noClustering/spA_mann_stabilityAssessment.tab": "name\tscore\nnumClusters\tNA\nclust1\tNA\n",
        "spC_mann_clustering.tab": "clust\ns0\t1\n",
        "spC_mann_distMatrixUsedForClustMedoidDefns.txt": used(6),
        "clustMedoidDefnFailed/spD_mann_clustering.tab": "clust\n",            # not a directory the summary reads
    }


CSV = ('"","speciesID","speciesName","numberOfSamplesUsedForClusterDetection","numberOfClusters","predictionStrengthValue","confidenceInNumberOfClusters",'
       '"confidencePerCluster","clusterSizes","detailedClusteringResultsFile"\n'
       '"spA","spA",NA,10,1,1,NA,"NA","10","./noClustering/spA_detailedSpeciesReport.html"\n'
       '"spB","spB",NA,12,2,0.9123,"Medium","High-NA","7-5","./spB_detailedSpeciesReport.html"\n'
       '"spC","spC",NA,6,1,NA,NA,NA,NA,"./spC_detailedSpeciesReport.html"\n')


def test_text_of_the_summary():
    assert model.summary_csv(project()) == CSV


def write_project(root):
    for rel, text in project().items():
        p = os.path.join(str(root), rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(text)


def test_summarise_clustering_writes_the_models_text(tmp_path):
    write_project(tmp_path)
    rows = subpopr.summarise_clustering(str(tmp_path))
    assert [r["speciesID"] for r in rows] == ["spA", "spB", "spC"]
    assert open(str(tmp_path / "summary_clustering.csv")).read() == CSV


def test_k_comes_from_the_ps_values(tmp_path):
    write_project(tmp_path)
    assert subpopr.clusters_from_ps_values(str(tmp_path), "spB") == 2 and subpopr.clusters_from_ps_values(str(tmp_path), "spB", 0.95) == 1
    assert subpopr.clusters_from_ps_values(str(tmp_path), "spB", 0.4) == 3 and subpopr.clusters_from_ps_values(str(tmp_path), "spC") == 1


# ---------------------------------------------------------------------------------- the launchers
def test_summary_launcher_completes(tmp_path):
    write_project(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "summariseClustering.py"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "summary_clustering.csv")).read() == CSV


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_stability_launcher_refuses_to_run_without_a_gpu(tmp_path):
    write_project(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "clusterMembStability.py"), "spB", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert open(str(tmp_path / "spB_mann_stabilityAssessment.tab")).read() == project()["spB_mann_stabilityAssessment.tab"]
