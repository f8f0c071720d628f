"""tests/genotypemodel.py, the numpy restatement the GPU genotyping tests compare with (tests/test_gpu_genotype.py), pinned on its own by
hand-worked tables: every condition of computeUniquePosPerCluster, the 20 % boundary, a cluster without coverage, the flip rule's tie, the
strict threshold, the exact text of every ending of <species>_hap_out.txt, and the launcher's refusal to run without a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import genotypecases as cases
import genotypemodel as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = np.nan


def masks(rows, clust, threshold=80.0):
    select, flip, _ = model.genotype_rows(np.array(rows, dtype=np.float64), clust, threshold)
    return select.tolist(), flip.tolist()


def test_six_samples_two_clusters_every_condition_decides_a_row():
    clust = [1, 1, 1, 2, 2, 2]
    rows = [
        [100, 100, 100, 0, 0, 0],        # means 100 and 0: both clusters; cluster 2 sits below 50: flipped
        [NA, 100, 100, 0, 0, 0],         # 1 of 3 NA: condition 1 drops cluster 1, condition 2 (its non-cluster columns) drops cluster 2
        [90, 90, 90, 10, 10, 10],        # a difference of exactly 80 is not above 80: condition 3
        [90.5, 90.5, 90.5, 10, 10, 10],  # 80.5 is
        [0, 0, 100, 100, 100, 100],      # 33.3 against 100: condition 3
        [10, 20, 0, 100, 95, 99],        # 10 against 98: both; cluster 1 flipped
        [100, 100, 100, 0, NA, 0],       # the NA on the other side: condition 1 drops cluster 2, condition 2 drops cluster 1
    ]
    assert masks(rows, clust) == ([3, 0, 0, 3, 0, 3, 0], [2, 0, 0, 2, 0, 1, 0])


def test_a_fifth_of_na_is_not_below_a_fifth():
    clust = [1] * 5 + [2] * 6
    one_of_five = [NA, 100, 100, 100, 100] + [0] * 6                 # 1 / 5 = 0.2, not < 0.2: cluster 1 by condition 1, cluster 2 by condition 2
    one_of_six = [100] * 5 + [NA, 0, 0, 0, 0, 0]                     # 1 / 6 < 0.2: kept on both sides
    assert masks([one_of_five, one_of_six], clust) == ([0, 3], [0, 2])


def test_a_cluster_without_a_cell_makes_no_candidate():
    clust = [1] * 10 + [2] * 10 + [3]
    # cluster 3 is all NA: 1 NA of 11 non-cluster columns passes condition 2 for clusters 1 and 2, but their difference to a NaN mean counts as 0
    assert masks([[100] * 10 + [0] * 10 + [NA]], clust) == ([0], [0])
    # with a cell there, cluster 1 is 100 away from both others; clusters 2 and 3 do not differ from each other
    assert masks([[100] * 10 + [0] * 10 + [0]], clust) == ([1], [0])


def test_as_many_below_50_as_not_is_no_flip():
    clust = [1, 1, 1, 1, 2, 2, 2, 2]
    rows = [[0, 0, 100, 100, 100, 100, 100, 100],                    # two and two: the median of 0 0 1 1 is 0.5, no flip
            [0, 0, 0, 100, 100, 100, 100, 100],                      # three and one: flipped
            [0, 0, 50, 50, 100, 100, 100, 100]]                      # 50 counts as the major allele: two and two
    assert masks(rows, clust, threshold=20.0) == ([3, 3, 3], [0, 1, 0])


def test_columns_not_in_use_are_not_read():
    clust = [0, 1, 1, 1, 0, 2, 2, 2]
    assert masks([[NA, 100, 100, 100, 55, 0, 0, 0], [0, 100, 100, 100, NA, NA, 0, 0]], clust) == ([3, 0], [2, 0])


def test_the_mean_is_the_long_double_one():
    # a cluster whose mean is 0.6 up to the rounding of its sum against one at 80.6: the row sits on the threshold, and the side it falls on
    # is the one the sequential long double sum, rounded to double, gives
    clust = [1, 1, 1, 2, 2, 2]
    row = [0.3, 0.6, 0.9, 80.6, 80.6, 80.6]
    m1 = model.cluster_means(np.array([row]), np.array(clust), 1)[0][0]
    assert m1 == float((np.longdouble(0.3) + np.longdouble(0.6) + np.longdouble(0.9)) / np.longdouble(3))
    select, _, near = model.genotype_rows(np.array([row]), clust)
    assert near.tolist() == [True]
    assert select.tolist() == [3 if abs(m1 - 80.6) > 80.0 else 0]


def test_planted_tables_have_their_positions_and_no_near_row():
    for s, k in ((6, 2), (64, 3), (129, 15), (300, 32)):
        table, clust = cases.planted_genotypes(s, k, 8, 40, 5, na_share=0.02)
        select, flip, near = model.genotype_rows(table, clust, guard=2e-6)
        assert not near.any()
        assert (select[8 * k:] == 0).all()                            # the background rows select nothing
        if s >= 64:
            found = sum(int(select[8 * c + r] >> c & 1) for c in range(k) for r in range(8))
            assert found > 4 * k, (s, k, found)                      # most planted rows (a small cluster loses a row to one NaN)
            assert all(int(flip[8 * c + r] >> c & 1) == r % 2 for c in range(k) for r in range(8) if select[8 * c + r] >> c & 1)


NAMES6 = list("abcdef")
CLUST6 = model.clustering_text(zip(NAMES6, [1, 1, 1, 2, 2, 2]))
ROWS_OK = [[1, 1, 1, 0, 0, 0], [0.25, 0, 0, 1, 1, 0.75], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]]


def test_ending_ok_and_its_files():
    files, info = model.genotype_files(CLUST6, (NAMES6, ["L1", "L2", "L3"], ROWS_OK), "sp")
    assert info["status"] == model.OK and (info["n_clusters"], info["n_samples"], info["n_rows"], info["n_positions"], info["n_correct"], info["n_good"]) == (2, 6, 3, 4, 6, 6)
    assert sorted(files) == ["sp_1_hap_positions.tab", "sp_2_hap_positions.tab", "sp_hap_freq_mean.tab", "sp_hap_freq_median.tab", "sp_hap_out.txt"]
    assert files["sp_hap_out.txt"] == (
        "\nGenotyping-based assignment of discovery samples to clusters was correct for 6 samples. Determined any cluster assignment from genotyping SNVs for "
        "6 out of 6 samples. Of those samples without assignments: 0  had incoherect cluster assignments and 0 lacked coverage of genotyping SNVs.\n")
    assert files["sp_1_hap_positions.tab"] == "posId\tflip\n1\tL1\tFALSE\n2\tL2\tTRUE\n"
    assert files["sp_2_hap_positions.tab"] == "posId\tflip\n1\tL1\tTRUE\n2\tL2\tFALSE\n"
    # cluster 1: L1 as it is, L2 as 100 - x: a = (100, 75), f = (0, 25); cluster 2 the other way round
    want = "\ti\na\t87.5\t1\nb\t100\t1\nc\t100\t1\nd\t0\t1\ne\t0\t1\nf\t12.5\t1\na\t12.5\t2\nb\t0\t2\nc\t0\t2\nd\t100\t2\ne\t100\t2\nf\t87.5\t2\n"
    assert files["sp_hap_freq_mean.tab"] == want and files["sp_hap_freq_median.tab"] == want


def test_ending_single_cluster():
    files, info = model.genotype_files(model.clustering_text(zip(NAMES6, [1] * 6)), (NAMES6, ["L1"], ROWS_OK[:1]), "sp")
    assert info["status"] == model.SINGLE and files == {"sp_hap_out.txt": "Single cluster\n"}
    files, info = model.genotype_files(model.clustering_text([("x", 1), ("y", 2)]), (NAMES6, ["L1"], ROWS_OK[:1]), "sp")    # no common sample
    assert info["status"] == model.SINGLE and info["n_samples"] == 0 and files == {"sp_hap_out.txt": "Single cluster\n"}


def test_ending_no_positions():
    files, info = model.genotype_files(CLUST6, (NAMES6, ["L3"], ROWS_OK[2:]), "sp")
    assert info["status"] == model.NO_POSITIONS and files == {"sp_hap_out.txt": (
        "\nNo unique genotyping positions for species sp cluster 1 (species has 2 total clusters)\n"
        "No unique genotyping positions for species sp cluster 2 (species has 2 total clusters)\n"
        "No genotyping positions for  sp\n")}
    files, info = model.genotype_files(model.clustering_text(zip(NAMES6, [0, 0, 0, -1, -1, -1])), (NAMES6, ["L1"], ROWS_OK[:1]), "sp")
    assert info["status"] == model.NO_POSITIONS and files == {"sp_hap_out.txt": "\nNo genotyping positions for  sp\n"}


NAMES9 = list("abcdefghi")
CLUST9 = model.clustering_text(zip(NAMES9, [5, 5, 5, 2, 2, 2, 9, 9, 9]))


def test_ending_cluster_missing():
    files, info = model.genotype_files(CLUST9, (NAMES9, ["L1"], [[1, 1, 1, 0, 0, 0, 0, 0, 0]]), "sp")
    assert info["status"] == model.CLUSTER_MISSING and info["n_positions"] == 1
    assert files == {"sp_5_hap_positions.tab": "posId\tflip\n1\tL1\tFALSE\n", "sp_hap_out.txt": (
        "\nNo unique genotyping positions for species sp cluster 2 (species has 3 total clusters)\n"
        "No unique genotyping positions for species sp cluster 9 (species has 3 total clusters)\n"
        "At least one cluster is missing genotyping positions for  sp . Aborting, but this could be fixed.\n")}


ROWS_BAD = [[1, 1, 1, 1, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 1, 1]]


def test_ending_cutoff_bad():
    # at a threshold of 50: L1 genotypes the first cluster (100 against 33.3 and 0), L2 the second, L3 the third; samples a and d carry both
    # L1 and L2 and sum to 200, 2 of 9 samples is more than 15 %
    files, info = model.genotype_files(CLUST9, (NAMES9, ["L1", "L2", "L3"], ROWS_BAD), "sp", uniq_threshold=0.5)
    assert info["status"] == model.CUTOFF_BAD
    assert files["sp_hap_out.txt"] == (
        "\nCutoff is bad\n"
        "In  2  out of  9  samples,  the summed abundance of all clusters per sample is >120% or < 80%,  based on the frequencies of the genotyping SNVs.\n"
        "Samples with incoherent cluster abundance measured based on genotyping SNVs: \na\nd\n")
    assert sorted(files) == ["sp_2_hap_positions.tab", "sp_5_hap_positions.tab", "sp_9_hap_positions.tab", "sp_hap_out.txt"]


def test_correct_assignments_compare_the_cluster_id_with_the_column_index():
    # the same table with one mixed sample only (1 of 9 is under 15 %): the ids are 5, 2, 9, the columns 1, 2, 3 -- only the second cluster's
    # samples "agree", as in the reference; sample a has no coverage on L3 (1 of 6 non-cluster columns) and no classification
    rows = [r[:] for r in ROWS_BAD]
    rows[1][0] = 0
    rows[2][0] = NA
    files, info = model.genotype_files(CLUST9, (NAMES9, ["L1", "L2", "L3"], rows), "sp", uniq_threshold=0.5)
    assert info["status"] == model.OK and info["n_good"] == 7 and info["n_correct"] == 2
    assert files["sp_hap_out.txt"] == (
        "\nGenotyping-based assignment of discovery samples to clusters was correct for 2 samples. Determined any cluster assignment from genotyping SNVs for "
        "7 out of 9 samples. Of those samples without assignments: 1  had incoherect cluster assignments and 1 lacked coverage of genotyping SNVs.\n")
    assert "a\tNA\t9\n" in files["sp_hap_freq_median.tab"] and "a\tNaN\t9\n" in files["sp_hap_freq_mean.tab"]


def test_inputs_the_stage_refuses():
    with pytest.raises(model.DomainError):
        model.genotype_files(CLUST6, (NAMES6, ["L1"], [[1.5, 1, 1, 0, 0, 0]]), "sp")
    with pytest.raises(model.FormatError):
        model.genotype_files(CLUST6.replace("c\t1", "c\tNA"), (NAMES6, ["L1"], ROWS_OK[:1]), "sp")


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_launcher_refuses_to_run_without_a_gpu(tmp_path):
    clustering, freq, out = tmp_path / "sp_mann_clustering.tab", tmp_path / "sp.filtered.freq", tmp_path / "out"
    clustering.write_text(CLUST6)
    cases.write_freq(str(freq), NAMES6, ["L1", "L2", "L3"], ROWS_OK)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "writeGenotypeFreqs.py"), "sp", str(clustering), str(freq), str(out)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert not out.exists()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "writeGenotypeFreqs.py"), "sp", str(clustering), str(tmp_path / "nosuch.freq"), str(out)], capture_output=True, text=True)
    assert r.returncode != 0 and "missing input file" in r.stderr
