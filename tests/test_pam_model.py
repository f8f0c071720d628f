"""tests/pammodel.py, the numpy restatement the GPU clustering tests compare with (tests/test_gpu_cluster.py), pinned on its own: hand-worked
PAM cases with every tie rule, local and exhaustive optimality, predStrengthCustom's last-entry quirk, planted clusters, the stability score,
the layout of _clustering.tab against the reference tutorial's file, and the launcher's refusal to run without a device.  The results the GPU
tests lean on at 1755, 1756 and 4096 members are checked by brute force, and the band table of the frequency-composition cases is shown to
tell the strict rule from a lenient one."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import pamcases as cases
import pammodel as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(xs):
    x = np.asarray(xs, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


def test_five_points_on_a_line_build_tie_takes_the_last():
    # BUILD: the row sums are 24 21 20 28 31 -> object 2; then beter = 2 2 . 16 16: objects 3 and 4 tie and the LAST wins -> {2, 4}, sky 4.
    # SWAP: (h = 1, i = 2) gives {1, 4} at cost 3, dz = -1, the only improvement; from there nothing is below 0.
    med, clus, swaps = model.pam(line([0, 1, 2, 10, 11]), 2)
    assert med.tolist() == [1, 4] and clus.tolist() == [1, 1, 1, 2, 2] and swaps == 1


def test_five_points_with_duplicates_every_tie_rule():
    # x = 0 0 2 4 4.  BUILD: object 2 (row sum 8), then beter = 4 4 . 4 4 -> the last, object 4: {2, 4}, sky 4.
    # SWAP: (h 0, i 2) and (h 1, i 2) both give dz = -2; the FIRST in (h, i) order wins -> {0, 4}, sky 2, then nothing improves.
    # Assignment: object 2 is 2 away from both medoids and goes to the FIRST.
    med, clus, swaps = model.pam(line([0, 0, 2, 4, 4]), 2)
    assert med.tolist() == [0, 4] and clus.tolist() == [1, 1, 1, 2, 2] and swaps == 1


def test_six_points_first_medoid_tie_and_no_swap():
    # x = 0 1 5 9 10 5.  BUILD: objects 2 and 5 share the smallest row sum (18): the last, 5; then beter = 8 8 0 8 8 -> object 4.
    # Every single swap of {4, 5} costs 10 or more, the cost it has: no swap.  Cluster 1 is medoid 4's (ascending medoid position).
    med, clus, swaps = model.pam(line([0, 1, 5, 9, 10, 5]), 2)
    assert med.tolist() == [4, 5] and clus.tolist() == [2, 2, 2, 1, 1, 2] and swaps == 0


def test_one_cluster_is_the_object_with_the_smallest_row_sum():
    d = cases.planted_dist(17, 0, 5)
    med, clus, swaps = model.pam(d, 1)
    sums = d.sum(axis=1)
    assert sums[med[0]] == sums.min() and clus.tolist() == [1] * 17 and swaps == 0


def test_no_single_swap_improves_and_the_optimum_is_usually_reached():
    rng = np.random.default_rng(11)
    optimal = 0
    for _ in range(30):
        d = cases.manhattan(rng.uniform(0, 1, size=(12, 2)))
        med, clus, _ = model.pam(d, 3)
        have = model.cost(d, med)
        for out in range(3):
            for h in set(range(12)) - set(med.tolist()):
                trial = [m for c, m in enumerate(med) if c != out] + [h]
                assert model.cost(d, trial) >= have - 1e-12
        best = min(model.cost(d, c) for c in itertools.combinations(range(12), 3))
        optimal += have <= best + 1e-12
        assert (clus == np.argmin(d[med], axis=0) + 1).all()
    assert optimal >= 24, optimal


def test_the_matrix_filled_in_blocks_is_the_manhattan_matrix():
    a = cases.planted_dist_blocks(300, 4, 21)                      # a second block of 44 rows
    assert a.tobytes() == cases.planted_dist(300, 4, 21, n_pos=12, noise=30.0).tobytes()
    for kind in ("real1756", "integer1756", "real4096"):           # what check_matrix asks for
        d = cases.large_matrix(kind)
        assert (d == d.T).all() and (np.diag(d) == 0).all() and np.isfinite(d).all() and (d >= 0).all(), kind


@pytest.mark.parametrize("kind,m,k", cases.LARGE_PAM)
def test_the_large_results_are_local_optima(kind, m, k):
    # The GPU tests at 1755, 1756 and 4096 members rest on the model alone, so here is what it gives checked without it: the cost recomputed
    # with numpy's own (pairwise) sums, and every exchange of one medoid for one non-medoid by brute force.  The model's sums over the m members
    # are sequential, numpy's pairwise: the two differ by less than m * 2^-52 * cost (each of m - 1 additions rounds by at most 2^-53 of a
    # partial sum no larger than the cost, in either order), so an exchange the model had to take would show as a gain above that.
    ix = cases.large_members(kind, m)
    d = cases.large_matrix(kind)[np.ix_(ix, ix)]
    med, clus, _ = cases.large_want(kind, m, k)
    assert len(set(med.tolist())) == k and (np.diff(med) > 0).all() and (clus == np.argmin(d[med], axis=0) + 1).all()
    have = np.min(d[med], axis=0).sum()
    others = np.setdiff1d(np.arange(m), med)
    best = np.inf
    for out in range(k):
        rest = np.min(d[np.delete(med, out)], axis=0) if k > 1 else np.full(m, np.inf)
        best = min(best, np.minimum(d[others], rest[None, :]).sum(axis=1).min())      # every h in the place of medoid `out`
    assert len(others) * k == (m - k) * k and best >= have - m * 2.0 ** -52 * have, (have, best)


@pytest.mark.parametrize("s,n_pos", [(255, 511), (256, 512), (257, 513), (600, 1100)])
def test_the_band_table_tells_the_strict_rule_from_a_lenient_one(s, n_pos):
    table = cases.band_table(n_pos, s, 50 + s)
    nan = cases.band_nan_column(s)
    assert table.shape == (n_pos, s) and np.isnan(table[:, nan]).all() and (nan == 256) == (s > 256)
    valid = [c for c in range(s) if c != nan]
    assert not np.isnan(table[:, valid]).all(axis=0).any() and np.isnan(table[:, valid]).any()
    for b in range(0, s, 256):                                     # every edge in every block of 256 columns, and not only in the NaN column
        cols = [c for c in range(b, min(b + 256, s)) if c != nan]
        for edge in cases.BAND_EDGES + (4.999, 95.001):            # (s = 257: the second block is the NaN column alone)
            assert (table[:, cols] == edge).any() or not cols, (b, edge)
    for p in range(0, n_pos, 512):                                 # and in every block row of 512 positions
        for edge in cases.BAND_EDGES:
            assert (table[p:p + 512, valid] == edge).any(), (p, edge)
    with np.errstate(invalid="ignore"):
        for c in valid:
            x = table[~np.isnan(table[:, c]), c]
            strict = model.freq_bands(table[:, c])
            lenient = [((x <= lo) | (x >= hi)).sum() / len(x) for lo, hi in ((20, 80), (10, 90), (5, 95))]
            assert all(a < b for a, b in zip(strict, lenient)), c  # a kernel with <= or >= would write another number in every column
    assert all(v != v for v in model.freq_bands(table[:, nan]))


def test_a_header_only_table_gives_nan_in_every_row():
    names = cases.sample_names(5)
    files, info = model.cluster_files(names, cases.planted_dist(5, 0, 3), "sp", freq=(names[:3] + ["x"], cases.band_table(0, 4, 1)))
    assert info["status"] == 3 and files == {"clustMedoidDefnFailed/sp_freq_composition.tab":
        "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95\n" + "".join(n + "\tNaN\tNaN\tNaN\n" for n in names[:3] + ["x"])}


def test_the_last_entry_of_a_half_is_left_out_of_the_numerator_only():
    # halves 0 1 10 11 | 0.5 1.5 10.5 11.5, k = 2: each half clusters as (1 1 2 2) and is classified the same way by the other's medoids.
    # Cluster 2 has nik = 2 but a holds only its first member: (1 - 1) / 2 = 0, where the textbook statistic would be 1.
    d = line([0, 1, 10, 11, 0.5, 1.5, 10.5, 11.5])
    assert model.split_strength(d, list(range(8)), 2) == 0.0
    # halves of 6: cluster 1 scores (9 - 3) / 6 = 1, cluster 2 has a = 2 of its 3 members: (4 - 2) / 6
    d = line([0, 1, 2, 10, 11, 12, 0.5, 1.5, 2.5, 10.5, 11.5, 12.5])
    assert model.split_strength(d, list(range(12)), 2) == 2.0 / 6.0
    # the same samples in an order that puts a member of cluster 1 last: now cluster 1 loses one and scores (4 - 2) / 6, cluster 2 scores 1
    order = [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]
    assert model.split_strength(d, order, 2) == 2.0 / 6.0


def test_classification_takes_the_first_medoid_on_ties():
    # half 2 = 0 0.5 4 4.5: BUILD takes object 2 (the last of the two row sums of 8), then object 1 (beter 7 7 . 0.5, the last): medoids at 0.5 and 4
    d = line([0, 0.25, 2.25, 4, 0, 0.5, 4, 4.5])
    med, clus, swaps = model.pam(d[4:, 4:], 2)
    assert med.tolist() == [1, 2] and clus.tolist() == [1, 1, 2, 2] and swaps == 0
    # half 1's member at 2.25 is 1.75 away from both and goes to the first; the others are clear
    assert d[2, 5] == d[2, 6] == 1.75
    assert model.classify(d, [0, 1, 2, 3], [5, 6]).tolist() == [0, 0, 0, 1]
    assert model.classify(d, [0, 1, 2, 3], [6, 5]).tolist() == [1, 1, 0, 0]


def test_planted_clusters_are_found():
    d = cases.planted_dist(120, 3, 1)
    _, mean_pred, k = model.run_strength(d, list(range(120)), model.max_clusters_to_try(120, 15, 3), 6, 1, 0, 0.8)
    assert k == 3 and mean_pred[2] > 0.8 and (mean_pred[3:] <= 0.8).all(), mean_pred
    d = cases.planted_dist(60, 2, 2)
    _, mean_pred, k = model.run_strength(d, list(range(60)), model.max_clusters_to_try(60, 15, 3), 6, 1, 0, 0.8)
    assert k == 2 and (mean_pred[2:] <= 0.8).all(), mean_pred


def test_r_mean_is_a_long_double_mean_with_a_second_pass():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    for n in (2, 3, 50):
        x = (rng.integers(0, 1000, size=n) / 977.0).tolist()
        assert model.r_mean(x) == float(sum(Fraction(v) for v in x) / n)      # correctly rounded, where a double sum / n is not always
    assert model.r_mean([1.0, 1.0, 1.0]) == 1.0 and model.r_sd([2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0]) == pytest.approx(2.138089935299395, abs=1e-15)


def test_the_draws_are_a_function_of_seed_and_ordinal():
    assert model.mix(0) == 0xe220a8397b1dcdaf                   # splitmix64's first output from state 0
    p = model.permutation(7, 3, 50)
    assert sorted(p) == list(range(50)) and p == model.permutation(7, 3, 50)
    assert p != model.permutation(7, 4, 50) and p != model.permutation(8, 3, 50)


def test_stability_score():
    props = [0.8, 0.8, 0.9, 0.9, 1.0000000000000002, 1.0000000000000002]
    assert model.stab_score(props, [3, 3, 3, 3, 3, 3]) == 3
    assert model.stab_score(props, [2, 3, 3, 3, 3, 3]) == 2    # 80 % varies: Medium
    assert model.stab_score(props, [3, 3, 2, 2, 3, 3]) == 2    # 90 % constant at another number: Medium
    assert model.stab_score(props, [3, 3, 3, 3, 3, 2]) == 1    # 100 % varies: Low
    assert model.stab_score(props, [3, 3, 3, 3, None, 3]) == 1  # an NA is not a constant group


def test_gmax_follows_the_smaller_half_and_the_cluster_size():
    assert [model.max_clusters_to_try(n, 15, 3) for n in (4, 5, 6, 9, 40, 120)] == [1, 1, 2, 3, 13, 15]
    assert [model.max_clusters_to_try(n, 10, 5) for n in (9, 12, 36, 120)] == [1, 2, 7, 10]


def test_clustering_tab_has_the_reference_layout(golden_dir):
    want = open(os.path.join(golden_dir, "subpopr", "cluster", "refGenome3clus_mann_clustering.tab")).read()
    rows = [ln.split("\t") for ln in want.splitlines()[1:]]
    assert want.splitlines()[0] == "clust" and len(rows) > 100
    assert model.clustering_text([r[0] for r in rows], [int(r[1]) for r in rows]) == want


def test_the_stage_on_a_small_table():
    # 5 samples: Gmax = min(5 // 2 - 1, 5 // 3) = 1, medoid definition fails: one cluster, the matrix in both directories, no PS values
    names = cases.sample_names(9)
    files, info = model.cluster_files(names[:5], cases.planted_dist(5, 0, 3), "sp", stability_iters=2)
    assert info["status"] == 2 and sorted(files) == ["clustMedoidDefnFailed/sp_mann_distMatrixUsedForClustMedoidDefns.txt", "noClustering/sp_mann_clustering.tab",
                                                      "noClustering/sp_mann_distMatrixUsedForClustMedoidDefns.txt"]
    assert files["noClustering/sp_mann_clustering.tab"] == "clust\n" + "".join(n + "\t1\n" for n in names[:5])


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_launcher_refuses_to_run_without_a_gpu(tmp_path):
    dist = tmp_path / "sp.filtered.mann.dist"
    cases.write_dist(str(dist), cases.sample_names(12), cases.planted_dist(12, 2, 1))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "clusterSubpops.py"), str(dist), str(out)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert not out.exists()
