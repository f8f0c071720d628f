"""subpopr's clustering on the device (csrc/cluster_k.hip, csrc/cluster.cpp) against tests/pammodel.py.  Every comparison is exact: integers
equal, doubles bit-equal, files byte-equal.

msnv_pam_tasks_k has one route (no size switches it): a workgroup of 256 lanes per task, the sub-matrix read through the task's index list.
The task sizes are those where its loops change shape: 2 and 3 (the smallest), 63 / 64 / 65 (a wavefront of BUILD candidates), 129 (more
than two wavefronts of candidates, several (h, i) pairs per lane), each with k = 1 (no SWAP), 2, 5 and m - 1.

A 9-sample table ends in clustMedoidDefnFailed/ the only way it can: getMaxNumClustersToTry gives 3 for 9 samples, so it is the frequency
filter that fails there (5 samples left, fewer than 6); the Gmax <= 1 route into the same directory is run with 5 samples."""
import os

import numpy as np
import pytest

import pamcases as cases
import pammodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EFORMAT, CLUSTER_OK, CLUSTER_NONE, CLUSTER_MEDOID_FAILED, CLUSTER_TOO_FEW

pytestmark = pytest.mark.gpu
N = 140
SIZES = (2, 3, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def matrix(kind):
    return cases.planted_dist(N, 4, 21, noise=30.0) if kind == "real" else cases.integer_dist(N, 22)


def size_tasks(seed):
    rng = np.random.default_rng(seed)
    return [(rng.choice(N, size=m, replace=False).astype(np.int32), k) for m in SIZES for k in sorted({1, 2, 5, m - 1}) if k < m]


_want = {}


def want_of(kind, d, task):
    key = (kind, task[0].tobytes(), task[1])
    if key not in _want:
        _want[key] = model.pam(d[np.ix_(task[0], task[0])], task[1])
    return _want[key]


def same(got, want):
    return got["medoids"].tolist() == want[0].tolist() and got["cluster"].tolist() == want[1].tolist() and got["n_swaps"] == want[2]


@pytest.mark.parametrize("kind", ["real", "integer"])
def test_pam_at_every_size(ctx, kind):
    d = matrix(kind)
    tasks = size_tasks(5)
    got, ms = subpopr.pam_tasks(ctx, d, tasks)
    assert ms > 0 and len(got) == len(tasks)
    swaps = 0
    for t, g in zip(tasks, got):
        w = want_of(kind, d, t)
        assert same(g, w), (kind, len(t[0]), t[1], g, w)
        swaps += g["n_swaps"]
    assert swaps > 0                                               # SWAP did run
    if kind == "integer":                                          # duplicated samples: zero distances inside the tasks
        assert any((d[np.ix_(t[0], t[0])] == 0).sum() > len(t[0]) for t in tasks)


@pytest.mark.parametrize("kind", ["real", "integer"])
def test_a_batch_larger_than_the_grid_gives_each_task_its_own_result(ctx, kind):
    d = matrix(kind)
    base = size_tasks(5)
    rng = np.random.default_rng(9)
    small = [(rng.choice(N, size=m, replace=False).astype(np.int32), k) for m, k in ((2, 1), (3, 2), (5, 2), (9, 3), (17, 4), (33, 5))]
    order = rng.permutation(4400)                                  # 2048 workgroups at the most are resident (256 CUs x 8)
    pool = base + small
    tasks = [pool[i % len(pool)] if i % 40 == 0 else small[i % len(small)] for i in order]
    got, _ = subpopr.pam_tasks(ctx, d, tasks)
    for t, g in zip(tasks, got):
        assert same(g, want_of(kind, d, t)), (len(t[0]), t[1])


@pytest.mark.parametrize("n,kind", [(13, "integer"), (64, "real"), (121, "real"), (121, "integer")])
def test_prediction_strength(ctx, n, kind):
    d = cases.planted_dist(n, 3, 30 + n, noise=20.0) if kind == "real" else cases.integer_dist(n, 31 + n)
    rng = np.random.default_rng(n)
    perms = np.array([[rng.permutation(n) for _ in range(3)] for _ in range(2, 6)], dtype=np.int32)
    got = subpopr.prediction_strength(ctx, d, 5, perms, cutoff=0.8)
    prederr, mean_pred, optimalk = model.pred_strength(d, 5, perms.tolist(), 0.8)
    print("n=%d %s: mean.pred %s" % (n, kind, mean_pred))
    assert got["prederr"].tobytes() == prederr.tobytes()
    assert got["mean_pred"].tobytes() == mean_pred.tobytes() and got["optimalk"] == optimalk


def read_tree(root):
    out = {}
    for dp, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p).read()
    return out


def run_stage(ctx, tmp_path, names, d, freq=None, **kw):
    os.makedirs(str(tmp_path), exist_ok=True)
    dist_path = str(tmp_path / "sp.filtered.mann.dist")
    cases.write_dist(dist_path, names, d)
    freq_path = None
    if freq is not None:
        freq_path = str(tmp_path / "sp.filtered.freq")
        cases.write_freq(freq_path, freq[0], freq[1])
    out = str(tmp_path / "out")
    res = subpopr.cluster_file(ctx, dist_path, out, freq_path=freq_path, stability_iters=2, **kw)
    files, info = model.cluster_files(names, d, "sp", freq=freq, stability_iters=2, seed=kw.get("seed", 1))
    got = read_tree(out) if os.path.isdir(out) else {}
    assert sorted(got) == sorted(files)
    for f in files:
        assert got[f] == files[f], f
    for key in ("status", "n_clusters", "n_samples", "n_outliers", "stability_score", "optimalk"):
        assert res[key] == info[key], key
    return res, got


def test_stage_three_planted_clusters(ctx, tmp_path):
    names = cases.sample_names(120)
    res, got = run_stage(ctx, tmp_path, names, cases.planted_dist(120, 3, 1))
    assert res["status"] == CLUSTER_OK and res["n_clusters"] == 3 and res["optimalk"] == 3 and res["stability_score"] >= 2
    rows = got["sp_mann_clustering.tab"].splitlines()
    assert rows[0] == "clust" and len(rows) == 121
    ids = [int(r.split("\t")[1]) for r in rows[1:]]
    assert all(len({ids[i] for i in range(g, 120, 3)}) == 1 for g in range(3)) and len(set(ids)) == 3      # the planted groups
    assert got["sp_mann_PS_values.tab"].startswith("x\n1\t1\n2\t")
    assert res["n_pam_tasks"] > 10000 and res["ms_kernel"] > 0


def test_stage_without_structure(ctx, tmp_path):
    names = cases.sample_names(40)
    res, got = run_stage(ctx, tmp_path, names, cases.planted_dist(40, 0, 4), seed=7)
    assert res["status"] == CLUSTER_NONE and res["n_clusters"] == 1
    assert got["noClustering/sp_mann_clustering.tab"] == "clust\n" + "".join(n + "\t1\n" for n in names)


def test_stage_medoid_definition_fails(ctx, tmp_path):
    # 9 samples, 4 of them mixed: 5 pass the frequency filter, fewer than 6 -> only the composition file, under clustMedoidDefnFailed/
    names = cases.sample_names(9)
    table = cases.planted_freqs(9, 2, 6)
    table[:4, ::2] = 50.0
    res, got = run_stage(ctx, tmp_path / "a", names, cases.manhattan(table), freq=(names, table.T))
    assert res["status"] == CLUSTER_TOO_FEW and sorted(got) == ["clustMedoidDefnFailed/sp_freq_composition.tab"]
    # 5 samples: Gmax = 1 -> one cluster, the matrix under clustMedoidDefnFailed/ as well
    res, got = run_stage(ctx, tmp_path / "b", names[:5], cases.planted_dist(5, 0, 3))
    assert res["status"] == CLUSTER_MEDOID_FAILED and "clustMedoidDefnFailed/sp_mann_distMatrixUsedForClustMedoidDefns.txt" in got


def test_stage_with_a_frequency_table_and_an_outlier(ctx, tmp_path):
    names = cases.sample_names(45)
    table = cases.planted_freqs(45, 2, 8)
    table[40:44, ::3] = 45.0                                       # four samples with a third of their SNVs mixed: below 0.8 at 10 / 90
    table[44] = 100.0 - table[44]                                  # one sample unlike every other: the outlier
    table[3, 5] = np.nan                                           # a position without coverage does not count
    order = list(np.random.default_rng(1).permutation(45))         # the freq table lists the samples in another order
    res, got = run_stage(ctx, tmp_path, names, cases.manhattan(np.nan_to_num(table, nan=0.0)), freq=([names[i] for i in order], table[order].T))
    assert res["n_outliers"] == 1 and res["n_samples"] == 40 and res["status"] == CLUSTER_OK and res["n_clusters"] == 2
    comp = got["sp_freq_composition.tab"].splitlines()
    assert comp[0] == "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95" and len(comp) == 46
    assert names[44] not in got["sp_mann_clustering.tab"] and names[41] not in got["sp_mann_clustering.tab"]


def test_inputs_outside_the_domain_are_refused(ctx, tmp_path):
    d = cases.planted_dist(12, 2, 1)
    ix = np.arange(6, dtype=np.int32)
    for bad in (-1.0, np.nan, np.inf):
        e = d.copy()
        e[2, 7] = e[7, 2] = bad
        with pytest.raises(MsnvError) as err:
            subpopr.pam_tasks(ctx, e, [(ix, 2)])
        assert err.value.code == EDOMAIN, bad
    e = d.copy()
    e[2, 7] += 1.0                                                 # not symmetric
    with pytest.raises(MsnvError) as err:
        subpopr.pam_tasks(ctx, e, [(ix, 2)])
    assert err.value.code == EDOMAIN
    for k in (6, 7, 0):
        with pytest.raises(MsnvError) as err:
            subpopr.pam_tasks(ctx, d, [(ix, k)])
        assert err.value.code == EDOMAIN, k
    with pytest.raises(MsnvError) as err:
        subpopr.pam_tasks(ctx, d, [(np.array([0, 1, 12], dtype=np.int32), 1)])
    assert err.value.code == EDOMAIN
    with pytest.raises(MsnvError) as err:                          # k_max must stay below the smaller half
        subpopr.prediction_strength(ctx, d, 6, np.zeros((5, 1, 12), dtype=np.int32))
    assert err.value.code == EDOMAIN
    names = cases.sample_names(12)
    path = str(tmp_path / "sp.filtered.mann.dist")
    cases.write_dist(path, names, d)
    text = open(path).read().replace(repr(float(d[2, 7])), "NA")
    open(path, "w").write(text)
    with pytest.raises(MsnvError) as err:
        subpopr.cluster_file(ctx, path, str(tmp_path / "out"))
    assert err.value.code == EFORMAT
    open(path, "w").write(text.replace("NA", ""))
    with pytest.raises(MsnvError) as err:
        subpopr.cluster_file(ctx, path, str(tmp_path / "out"))
    assert err.value.code == EFORMAT
