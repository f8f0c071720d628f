"""tests/hclustmodel.py, the rule the device is compared with bit for bit (tests/test_gpu_hclust.py), against what is known without it: trees
worked by hand, scipy's linkage on tie-free matrices, and the properties every hc$merge / hc$order and every reordered dendrogram has.  The
host-only entry msnv_heatmap_order is held to the model here, without a device.

The bound of the scipy comparison: a Lance-Williams update of average or McQuitty linkage rounds three times (two products or halvings that can
round, one sum, one quotient; scipy's form rounds as often in another order), and a cell is the result of at most m - 1 nested updates, so two
correct implementations differ by at most about 4 (m - 1) 2^-53 relative.  max and min round nowhere: complete and single heights are bit-equal."""
import numpy as np
import pytest

import hclustcases as cases
import hclustmodel as model
from metasnv_amd import subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EINVAL


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_worked_trees(name):
    d, by_method = cases.HAND[name]
    for method, (merge, height, order) in by_method.items():
        res = model.hclust(d, np.arange(d.shape[0]), method)
        assert res["merge"].tolist() == merge and res["height"].tolist() == height and res["order"].tolist() == order, (name, method)


def test_a_task_is_a_list_of_positions():
    d = cases.FIVE
    idx = [3, 0, 4, 1]                                             # positions 0..3 are these samples: d' = [[0, 8, 20, 9], [8, 0, 16, 1], [20, 16, 0, 15], [9, 1, 15, 0]]
    res = model.hclust(d, idx, model.COMPLETE)
    assert res["merge"].tolist() == [[-2, -4], [-1, 1], [-3, 2]] and res["height"].tolist() == [1, 9, 20] and res["order"].tolist() == [2, 0, 1, 3]


@pytest.mark.parametrize("m", (30, 120))
@pytest.mark.parametrize("method", model.METHODS)
def test_against_scipy_linkage(method, m):
    pytest.importorskip("scipy.cluster.hierarchy")
    d = cases.matrix("manhattan", m)
    assert cases.tie_free(d)
    res = cases.want("manhattan", m, method)
    rel = cases.check_against_scipy(d, res["merge"], res["height"], method)
    print("%s m=%d: heights within %.3g relative of scipy's (bound %.3g)" % (model.METHOD_NAMES[method], m, rel, 4 * (m - 1) * 2.0 ** -53))


@pytest.mark.parametrize("m", (2, 3, 5, 64, 65))
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("method", model.METHODS)
def test_merge_and_order_properties(method, kind, m):
    res = cases.want(kind, m, method)
    cases.check_tree(m, res)
    if kind == "integer" and m >= 64:
        d = cases.matrix(kind, m)
        assert not cases.tie_free(d) and (d == 0).sum() > m and res["height"][0] == 0.0      # zero distances between distinct samples


def check_reorder(merge, weights, order, kids, value):
    m = len(weights)

    def of(e):
        return weights[-e - 1] if e < 0 else value[e]
    for s in range(1, m):
        left, right = kids[s - 1]
        assert of(left) <= of(right)
        assert sorted((left, right)) == sorted(int(e) for e in merge[s - 1])
        if of(left) == of(right):
            assert [left, right] == [int(e) for e in merge[s - 1]]          # equal values keep their merge order
    assert sorted(order.tolist()) == list(range(m))


def test_reorder_by_hand():
    merge = np.array(cases._CHAIN5, dtype=np.int32)
    order, kids, value = model.reorder(merge, [5, 1, 2, 9, 3])
    # node 1: leaves 0 (5) and 1 (1) swap, 6; node 2: leaf 2 (2) before node 1 (6), 8; node 3: leaf 3 (9) behind node 2 (8), 17; node 4: leaf 4 (3), 20
    assert kids == [(-2, -1), (-3, 1), (2, -4), (-5, 3)] and value[1:] == [6, 8, 17, 20]
    assert order.tolist() == [4, 2, 1, 0, 3]
    order, kids, _ = model.reorder(merge, [1, 1, 2, 4, 8])          # 1 = 1, 2 = 2, 4 = 4, 8 = 8: nothing moves
    assert kids == [tuple(r) for r in cases._CHAIN5] and order.tolist() == [4, 3, 2, 0, 1]


@pytest.mark.parametrize("kind", cases.KINDS)
def test_reorder_properties(kind):
    m = 65
    d = cases.matrix(kind, m)
    merge = cases.want(kind, m, model.AVERAGE)["merge"]
    for weights in (model.row_means(d), np.ones(m), np.arange(m, 0, -1.0)):
        order, kids, value = model.reorder(merge, weights)
        check_reorder(merge, weights, order, kids, value)


def test_row_means_are_long_double_sums():
    sub = np.array([[0.0, 1.0, 2.0 ** -60, -1.0], [3.0, 0.0, 0.0, 0.0]])
    assert model.row_means(sub).tolist() == [2.0 ** -62, 0.75]      # a double sum would lose 2^-60 beside 1


def test_the_files_of_the_stage():
    import pamcases
    import pammodel
    names = pamcases.sample_names(5)
    used = pammodel.dist_text(names, cases.FIVE, [3, 0, 4, 1])
    clustering = pammodel.clustering_text([names[i] for i in (0, 1, 3)], [1, 1, 2])
    files, info = model.heatmap_files(names, cases.FIVE, "sp", used, clustering)
    assert info == {"status": model.OK, "n_samples": 5, "n_discovery": 4, "have_clustering": True}
    assert files["sp_mann_hclust_all.tab"] == "merge1\tmerge2\theight\n1\t-1\t-2\t1\n2\t-3\t1\t3.5\n3\t-4\t2\t9\n4\t-5\t3\t16.25\n"
    assert files["sp_mann_hclust_discovery.tab"] == "merge1\tmerge2\theight\n1\t-2\t-4\t1\n2\t-1\t1\t9\n3\t-3\t2\t20\n"
    # rowMeans of FIVE: 5.8, 5.6, 6.2, 9.4, 13; node 1 (0, 1) -> (1, 0), 11.4; node 2 (2, node 1), 17.6; node 3 (3, node 2), 27; node 4 (4, node 3)
    assert files["sp_mann_heatmap_all.tab"] == ("index\thclustPos\tinDiscoverySubset\tclust\n" + "s0005.bam\t5\t1\tTRUE\tNA\n" + "s0004.bam\t4\t2\tTRUE\t2\n"
                                                + "s0003.bam\t3\t3\tFALSE\tNA\n" + "s0002.bam\t2\t5\tTRUE\t1\n" + "s0001.bam\t1\t4\tTRUE\t1\n")
    # the subset (samples 3, 0, 4, 1): rowMeans 9.25, 6.25, 12.75, 6.25; node 1 (1, 3) equal: kept, 12.5; node 2 (0, node 1), 21.75; node 3 (2, node 2)
    assert files["sp_mann_heatmap_discovery.tab"] == ("index\thclustPos\tinDiscoverySubset\tclust\n" + "s0005.bam\t3\t1\tTRUE\tNA\n" + "s0004.bam\t1\t2\tTRUE\t2\n"
                                                      + "s0001.bam\t2\t3\tTRUE\t1\n" + "s0002.bam\t4\t4\tTRUE\t1\n")
    files, info = model.heatmap_files(names, cases.FIVE, "sp", None, None)
    assert sorted(files) == ["sp_mann_hclust_all.tab", "sp_mann_heatmap_all.tab"] and info["status"] == model.NO_DISCOVERY and not info["have_clustering"]
    assert [ln.split("\t")[3:] for ln in files["sp_mann_heatmap_all.tab"].splitlines()[1:]] == [["FALSE", "NA"]] * 5
    files, info = model.heatmap_files(names, cases.FIVE, "sp", names[2] + "\n" + names[2] + "\t0\n", None)      # one sample: no discovery tree
    assert info["status"] == model.NO_DISCOVERY and info["n_discovery"] == 0


# ---------------------------------------------------------------------------------------------- msnv_heatmap_order: host only, no device
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("m", (2, 5, 65))
def test_heatmap_order_equals_the_model(kind, m):
    d = cases.matrix(kind, m)
    for method in (model.AVERAGE, model.SINGLE):
        merge = cases.want(kind, m, method)["merge"]
        for weights in (model.row_means(d), np.ones(m), np.arange(m, 0, -1.0), np.random.default_rng(m).integers(0, 4, m).astype(np.float64)):
            assert subpopr.heatmap_order(merge, weights).tolist() == model.reorder(merge, weights)[0].tolist()
    merge = np.array(cases._CHAIN5, dtype=np.int32)
    assert subpopr.heatmap_order(merge, [5, 1, 2, 9, 3]).tolist() == [4, 2, 1, 0, 3]
    big = 2.0 ** 53                                                # sums that do not fit a double
    assert subpopr.heatmap_order(cases._TWO_PAIRS, [big, 1.0, 1.0, big + 2.0]).tolist() == model.reorder(np.array(cases._TWO_PAIRS), [big, 1.0, 1.0, big + 2.0])[0].tolist()


def test_heatmap_order_refuses_what_is_no_tree():
    w5 = [1.0] * 5
    for merge in ([[-1, -2], [-3, 1], [-4, 2], [-5, 2]],           # step 2 is a child twice, step 3 never
                  [[-1, -2], [-3, 2], [-4, 1], [-5, 3]],           # row 2 names itself
                  [[-1, -2], [-1, 1], [-4, 2], [-5, 3]],           # leaf 1 twice
                  [[-1, -2], [-3, 1], [-4, 2], [-6, 3]],           # a sixth leaf
                  [[-1, -2], [-3, 1], [-4, 2], [0, 3]],            # 0 is no label
                  [[-1, -2], [-3, 4], [-4, 2], [-5, 3]]):          # a later step
        assert not model.is_tree(5, merge)
        with pytest.raises(MsnvError) as e:
            subpopr.heatmap_order(merge, w5)
        assert e.value.code == EINVAL, merge
    assert model.is_tree(5, cases._CHAIN5)
    with pytest.raises(MsnvError) as e:
        subpopr.heatmap_order(np.zeros((0, 2), dtype=np.int32), [1.0])
    assert e.value.code == EINVAL
    for bad in (np.nan, np.inf):
        with pytest.raises(MsnvError) as e:
            subpopr.heatmap_order(cases._CHAIN5, [1.0, bad, 1.0, 1.0, 1.0])
        assert e.value.code == EDOMAIN


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_launcher_refuses_to_run_without_a_gpu(tmp_path):
    import os
    import subprocess
    import sys
    import pamcases
    names = pamcases.sample_names(5)
    dist = tmp_path / "sp.filtered.mann.dist"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "heatmapSubpops.py"), str(dist), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "missing input file" in r.stderr
    pamcases.write_dist(str(dist), names, cases.FIVE)
    r = subprocess.run([sys.executable, os.path.join(root, "heatmapSubpops.py"), str(dist), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert os.listdir(str(tmp_path)) == ["sp.filtered.mann.dist"]
