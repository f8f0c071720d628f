"""The agglomeration behind subpopr's report heatmaps on the device (csrc/hclust_k.hip, csrc/hclust.cpp) against tests/hclustmodel.py.  Every
comparison with the model is exact: integers equal, doubles bit-equal, files byte-equal.

The sizes are those where the kernel's loops change shape.  A task has one workgroup of T = 256 lanes (hclustcases.THREADS): the update of a step
gives lane t the positions t, t + T, ...; a rescan lays a row's columns along one wavefront of 64.  So: 2 (one step, nothing to update), 3 .. 5,
63 / 64 / 65 (a row of one wavefront pass, and one column more), T - 1 / T / T + 1 (a second position per lane).  At T + 1 and 2 T + 1 the
tie-free matrices are also held to scipy's linkage on the terms of tests/test_hclust_model.py, and every matrix to what any tree satisfies; so
are 2049 members, the first size at which the launch has to raise the dynamic-LDS limit (24 bytes a member against 48 KiB), and 4096, the cap."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hclustcases as cases
import hclustmodel as model
import pamcases
from metasnv_amd import core, subpopr
from metasnv_amd._lib import (MsnvError, EDOMAIN, EINVAL, CLUSTER_OK, CLUSTER_TOO_FEW, HEATMAP_OK, HEATMAP_NO_DISCOVERY, HCLUST_AVERAGE, HCLUST_COMPLETE,
                              HCLUST_SINGLE, HCLUST_MCQUITTY)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def same(got, want):
    assert got["merge"].dtype == np.int32 and got["order"].dtype == np.int32 and got["height"].dtype == np.float64
    assert got["merge"].tobytes() == np.ascontiguousarray(want["merge"], dtype=np.int32).tobytes()
    assert got["height"].tobytes() == np.ascontiguousarray(want["height"], dtype=np.float64).tobytes()
    assert got["order"].tobytes() == np.ascontiguousarray(want["order"], dtype=np.int32).tobytes()


def test_the_constants_are_the_models():
    assert (HCLUST_AVERAGE, HCLUST_COMPLETE, HCLUST_SINGLE, HCLUST_MCQUITTY) == model.METHODS and (HEATMAP_OK, HEATMAP_NO_DISCOVERY) == (model.OK, model.NO_DISCOVERY)


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_worked_trees(ctx, name):
    d, by_method = cases.HAND[name]
    for method, (merge, height, order) in by_method.items():
        got = subpopr.hclust_tasks(ctx, d, [(np.arange(d.shape[0]), method)])[0][0]
        assert got["merge"].tolist() == merge and got["height"].tolist() == height and got["order"].tolist() == order, (name, method)


@pytest.mark.parametrize("m", cases.MODEL_SIZES)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_hclust_at_every_size(ctx, kind, m):
    d = cases.matrix(kind, m)
    got, ms = subpopr.hclust_tasks(ctx, d, [(np.arange(m), method) for method in model.METHODS])
    print("%s m=%d: four methods, %.3f ms in the kernel" % (kind, m, ms))
    for method in model.METHODS:
        same(got[method], cases.want(kind, m, method))
    if kind == "integer" and m >= 63:
        assert not cases.tie_free(d) and got[0]["height"][0] == 0.0


@pytest.mark.parametrize("m", cases.SCIPY_SIZES)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_past_the_workgroup_against_scipy_and_as_a_tree(ctx, kind, m):
    pytest.importorskip("scipy.cluster.hierarchy")
    d = cases.matrix(kind, m)
    got, ms = subpopr.hclust_tasks(ctx, d, [(np.arange(m), method) for method in model.METHODS])
    print("%s m=%d: four methods, %.3f ms in the kernel" % (kind, m, ms))
    for method in model.METHODS:
        cases.check_tree(m, got[method])
        if kind == "manhattan":
            assert cases.tie_free(d)
            rel = cases.check_against_scipy(d, got[method]["merge"], got[method]["height"], method)
            print("  %s: heights within %.3g relative of scipy's (bound %.3g)" % (model.METHOD_NAMES[method], rel, 4 * (m - 1) * 2.0 ** -53))


@pytest.mark.parametrize("m,methods", [(cases.LDS_SWITCH, model.METHODS), (cases.CAP, (model.AVERAGE,))])
def test_past_48_kib_of_lds_and_at_the_cap(ctx, m, methods):
    """The launch raises the dynamic-LDS limit from 2049 members (24 bytes each); 4096 is the cap: 96 KiB of LDS, 128 MiB of scratch."""
    pytest.importorskip("scipy.cluster.hierarchy")
    d = cases.matrix("manhattan", m)
    got, ms = subpopr.hclust_tasks(ctx, d, [(np.arange(m), method) for method in methods])
    print("manhattan m=%d: %d method(s), %.1f ms in the kernel" % (m, len(methods), ms))
    for res, method in zip(got, methods):
        cases.check_tree(m, res)
        rel = cases.check_against_scipy(d, res["merge"], res["height"], method)
        print("  %s: heights within %.3g relative of scipy's (bound %.3g)" % (model.METHOD_NAMES[method], rel, 4 * (m - 1) * 2.0 ** -53))


def test_every_row_has_the_same_nearest_column(ctx):
    m = 130
    d = cases.same_nearest_column(m)
    assert (np.argmin(np.where(np.triu(np.ones((m, m), dtype=bool), 1), d, np.inf)[:-1], axis=1) == m - 1).all()
    got, _ = subpopr.hclust_tasks(ctx, d, [(np.arange(m), method) for method in model.METHODS])
    for method in model.METHODS:
        same(got[method], cases.want("same_nearest", m, method))
    assert got[HCLUST_COMPLETE]["merge"][:, 0].tolist() == [-1] + [-(m - s) for s in range(1, m - 1)]      # leaf 0 takes the last column, step after step


# ---------------------------------------------------------------------------------------------- a task's result is a function of the task alone
def mixed_batch(kind):
    n = 300
    d = cases.matrix(kind, n)
    rng = np.random.default_rng(77)
    sizes = [300, 2, 65, 3, 257, 17, 64, 100, 5, 130, 256, 31]
    return d, [(rng.permutation(n)[:m].astype(np.int32), model.METHODS[(t + t // 4) % 4]) for t, m in enumerate(sizes)]


def as_bytes(res):
    return [(r["merge"].tobytes(), r["height"].tobytes(), r["order"].tobytes()) for r in res]


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_task_alone_and_inside_a_mixed_batch(ctx, kind):
    d, tasks = mixed_batch(kind)
    assert {m for _, m in tasks} == set(model.METHODS)
    batch = as_bytes(subpopr.hclust_tasks(ctx, d, tasks)[0])
    for t, task in enumerate(tasks):
        alone = subpopr.hclust_tasks(ctx, d, [task])[0]
        assert as_bytes(alone) == [batch[t]], t
        if len(task[0]) <= 130:
            same(alone[0], model.hclust(d, task[0], task[1]))
    assert as_bytes(subpopr.hclust_tasks(ctx, d, tasks[::-1])[0]) == batch[::-1]


@pytest.mark.parametrize("kb", ("1", "600", "1500"))
def test_a_batch_cut_into_several_launches(ctx, monkeypatch, kb):
    """8 m^2 bytes per task: at 1 KB every task is a launch of its own, at 600 KB (300 members take 703 KB, 257 take 516 KB) small tasks share
    launches between the large ones, at 1500 KB a cut falls inside the batch once."""
    d, tasks = mixed_batch("integer")
    whole = as_bytes(subpopr.hclust_tasks(ctx, d, tasks)[0])
    monkeypatch.setenv("MSNV_HCLUST_SCRATCH_KB", kb)
    assert as_bytes(subpopr.hclust_tasks(ctx, d, tasks)[0]) == whole


def test_inputs_outside_the_domain_are_refused(ctx):
    d = cases.matrix("manhattan", 8)
    every = np.arange(8)

    def refused(dist, tasks, code):
        with pytest.raises(MsnvError) as err:
            subpopr.hclust_tasks(ctx, dist, tasks)
        assert err.value.code == code, (tasks, err.value)
    refused(np.zeros((1, 1)), [([0, 0], HCLUST_AVERAGE)], EDOMAIN)                # n = 1
    e = d.copy()
    e[2, 5] += 1.0
    refused(e, [(every, HCLUST_AVERAGE)], EDOMAIN)                               # not symmetric
    e = d.copy()
    e[2, 5] = e[5, 2] = np.nan
    refused(e, [(every, HCLUST_AVERAGE)], EDOMAIN)
    refused(d, [(every, HCLUST_AVERAGE), ([3], HCLUST_COMPLETE)], EDOMAIN)       # m = 1
    refused(d, [(every, HCLUST_AVERAGE), ([3, 5, 3], HCLUST_COMPLETE)], EDOMAIN)  # a repeated index
    refused(d, [([3, 8], HCLUST_COMPLETE)], EDOMAIN)                             # a sample the matrix does not hold
    refused(d, [(every, 4)], EINVAL)                                             # an unknown method
    refused(d, [(every, -1)], EINVAL)
    refused(d, [], EINVAL)                                                       # no task
    same(subpopr.hclust_tasks(ctx, d, [([3, 5], HCLUST_COMPLETE), ([5, 3], HCLUST_SINGLE)])[0][1], model.hclust(d, [5, 3], model.SINGLE))      # an index may return in another task


# ---------------------------------------------------------------------------------------------- the stage on files
def check_files(directory, files, info, res):
    for which in ("hclust_all", "heatmap_all", "hclust_discovery", "heatmap_discovery"):
        name = "sp_mann_%s.tab" % which
        path = os.path.join(directory, name)
        assert os.path.exists(path) == (name in files), name
        if name in files:
            assert open(path).read() == files[name], name
    for key, v in info.items():
        assert res[key] == v, key


def read_or_none(path):
    return open(path).read() if os.path.exists(path) else None


def model_files(names, d, directory):
    return model.heatmap_files(names, d, "sp", read_or_none(os.path.join(directory, "sp_mann_distMatrixUsedForClustMedoidDefns.txt")),
                               read_or_none(os.path.join(directory, "sp_mann_clustering.tab")))


def clustered(ctx, tmp_path, names, d, freq):
    dist_path = str(tmp_path / "sp.filtered.mann.dist")
    pamcases.write_dist(dist_path, names, d)
    freq_path = str(tmp_path / "sp.filtered.freq")
    pamcases.write_freq(freq_path, freq[0], freq[1])
    out = str(tmp_path / "out")
    return dist_path, out, subpopr.cluster_file(ctx, dist_path, out, freq_path=freq_path, stability_iters=2)


def test_stage_after_the_clustering(ctx, tmp_path):
    names, table, order, d = cases.stage_samples()
    dist_path, out, clus = clustered(ctx, tmp_path, names, d, ([names[i] for i in order], table[order].T))
    assert clus["status"] == CLUSTER_OK and clus["n_samples"] == 40
    before = sorted(os.listdir(out))
    res = subpopr.heatmap_file(ctx, dist_path, out)
    files, info = model_files(names, d, out)
    assert len(files) == 4 and info == {"status": model.OK, "n_samples": 45, "n_discovery": 40, "have_clustering": True}
    check_files(out, files, info, res)
    assert res["ms_kernel"] > 0 and sorted(os.listdir(out)) == sorted(before + list(files))      # nothing else written
    rows = [r.split("\t") for r in files["sp_mann_heatmap_all.tab"].splitlines()]
    assert rows[0] == ["index", "hclustPos", "inDiscoverySubset", "clust"] and sorted(r[0] for r in rows[1:]) == names
    assert sorted(int(r[1]) for r in rows[1:]) == list(range(1, 46)) and sorted(int(r[2]) for r in rows[1:]) == list(range(1, 46))
    by_name = {r[0]: r for r in rows[1:]}
    assert all(by_name[nm][3] == "FALSE" and by_name[nm][4] == "NA" for nm in names[40:]) and all(by_name[nm][3] == "TRUE" for nm in names[:40])
    header = open(os.path.join(out, "sp_mann_distMatrixUsedForClustMedoidDefns.txt")).readline().rstrip("\n").split("\t")
    rows = [r.split("\t") for r in files["sp_mann_heatmap_discovery.tab"].splitlines()[1:]]
    assert header != names[:40] and all(header[int(r[1]) - 1] == r[0] for r in rows)         # index counts in the subset's own order, the freq file's


def test_stage_without_a_discovery_subset(ctx, tmp_path):
    names = pamcases.sample_names(8)
    d = cases.matrix("manhattan", 8)
    table = np.full((8, 30), 45.0)                                  # no sample is homogeneous: the medoids cannot be defined
    dist_path, out, clus = clustered(ctx, tmp_path, names, d, (names, table.T))
    assert clus["status"] == CLUSTER_TOO_FEW
    directory = os.path.join(out, "clustMedoidDefnFailed")
    assert os.listdir(directory) == ["sp_freq_composition.tab"]
    res = subpopr.heatmap_file(ctx, dist_path, directory, species="sp")
    files, info = model_files(names, d, directory)
    assert sorted(files) == ["sp_mann_hclust_all.tab", "sp_mann_heatmap_all.tab"] and info["status"] == model.NO_DISCOVERY and not info["have_clustering"]
    check_files(directory, files, info, res)
    assert res["status"] == HEATMAP_NO_DISCOVERY and res["n_discovery"] == 0 and not res["have_clustering"]


def test_stage_refuses_files_that_do_not_fit(ctx, tmp_path):
    from metasnv_amd._lib import EFORMAT
    names = pamcases.sample_names(5)
    dist_path = str(tmp_path / "sp.filtered.mann.dist")
    pamcases.write_dist(dist_path, names, cases.FIVE)
    used = tmp_path / "sp_mann_distMatrixUsedForClustMedoidDefns.txt"
    for header in ("s0001.bam\ts0009.bam\ts0002.bam", "s0001.bam\ts0002.bam\ts0001.bam"):      # a name the matrix does not hold; a name twice
        used.write_text(header + "\n")
        with pytest.raises(MsnvError) as err:
            subpopr.heatmap_file(ctx, dist_path, str(tmp_path), species="sp")
        assert err.value.code == EFORMAT, header
    used.write_text("s0004.bam\r\n")                               # one sample, a carriage return: no discovery tree
    assert subpopr.heatmap_file(ctx, dist_path, str(tmp_path))["status"] == HEATMAP_NO_DISCOVERY
    text = open(dist_path).read().replace("\t16.0", "\tNA")
    open(dist_path, "w").write(text)
    assert "NA" in text
    with pytest.raises(MsnvError) as err:                          # rmNAfromDistMatrix is not built
        subpopr.heatmap_file(ctx, dist_path, str(tmp_path))
    assert err.value.code == EFORMAT


def test_the_launcher_writes_the_same_files(ctx, tmp_path):
    names, table, order, d = cases.stage_samples()
    dist_path, out, _ = clustered(ctx, tmp_path, names, d, ([names[i] for i in order], table[order].T))
    files, _ = model_files(names, d, out)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "heatmapSubpops.py"), dist_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Species sp: 45 samples ordered (average linkage); 40 of the discovery subset (complete linkage)" in r.stdout
    for name, text in files.items():
        assert open(os.path.join(out, name)).read() == text, name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "heatmapSubpops.py"), dist_path, str(tmp_path / "nowhere")], capture_output=True, text=True)
    assert r.returncode == 1 and "missing directory" in r.stderr
