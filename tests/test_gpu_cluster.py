"""subpopr's clustering on the device (csrc/cluster_k.hip, csrc/cluster.cpp) against tests/pammodel.py.  Every comparison is exact: integers
equal, doubles bit-equal, files byte-equal.

msnv_pam_tasks_k has one route (no size switches it): a workgroup of 256 lanes per task, the sub-matrix read through the task's index list.
The task sizes are those where its loops change shape: 2 and 3 (the smallest), 63 / 64 / 65 (a wavefront of BUILD candidates), 129 (more
than two wavefronts of candidates, several (h, i) pairs per lane), each with k = 1 (no SWAP), 2, 5 and m - 1.  What does change with the size
is the launch (run_batch): 28 bytes of dynamic LDS per member of the largest task, so 1755 members (49 140 B) stay under 48 KiB and 1756
(49 168 B) raise the kernel's limit; a large task among small ones sets the LDS layout of all of them; at 4096 members, the cap (114 688 B),
one workgroup fits a CU and the grid shrinks to one per CU.  The model's results at those sizes are checked on their own in
tests/test_pam_model.py.  msnv_ps_splits_k runs with halves of 256 / 257, 300 / 301 (its loops over 256 lanes make a second trip) and
1756 / 1757 (the large-LDS PAM inside the split launch); msnv_freq_bands_k at the edges of its grid of 256 columns x 512 positions, with
cells exactly on 5, 10, 20, 80, 90 and 95, a column without a valid cell and a header-only table.

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


def size_tasks(seed, n=N):
    rng = np.random.default_rng(seed)
    return [(rng.choice(n, size=m, replace=False).astype(np.int32), k) for m in SIZES for k in sorted({1, 2, 5, m - 1}) if k < m]


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


def large_task(kind, m, k):
    return (cases.large_members(kind, m), k)


@pytest.mark.parametrize("kind", ["real1756", "integer1756"])
def test_pam_on_both_sides_of_48_kib_of_lds(ctx, kind):
    # 1755 members: 49 140 bytes of dynamic LDS, the default limit holds; 1756: 49 168, the launch raises the kernel's limit first.  Every lane
    # has seven BUILD candidates; the integer matrix keeps ties and zero distances among them.
    d = cases.large_matrix(kind)
    swaps = 0
    for m in (1755, 1756):                                         # a launch each: lds_m is the task's own
        tasks = [large_task(kind, m, k) for k in (1, 2, 5)]
        got, ms = subpopr.pam_tasks(ctx, d, tasks)
        print("%s m=%d: %.1f ms in the kernel" % (kind, m, ms))
        for (_, k), g in zip(tasks, got):
            assert same(g, cases.large_want(kind, m, k)), (kind, m, k, g["medoids"], g["n_swaps"])
            swaps += g["n_swaps"]
    assert swaps > 0                                               # SWAP did run at these sizes
    if kind == "integer1756":
        assert (d == 0).sum() > 10 * d.shape[0]


@pytest.mark.parametrize("large_first", [True, False])
def test_a_large_task_among_small_ones_leaves_them_their_own_results(ctx, large_first):
    # lds_m is the large task's, so every small task lays its arrays out at the large one's offsets; three workgroups fit a CU
    d = cases.large_matrix("real1756")
    small = size_tasks(5, n=1756)
    tasks = [large_task("real1756", 1756, 5)] + small if large_first else small + [large_task("real1756", 1756, 5)]
    got, _ = subpopr.pam_tasks(ctx, d, tasks)
    big = got.pop(0 if large_first else -1)
    assert same(big, cases.large_want("real1756", 1756, 5)) and big["n_swaps"] > 0
    for t, g in zip(small, got):
        assert same(g, want_of("real1756", d, t)), (len(t[0]), t[1])


@pytest.mark.parametrize("k", [1, 3])
def test_pam_at_the_cap_alone_and_among_600_small_tasks(ctx, k):
    # 4096 members: 114 688 bytes of dynamic LDS and 3 080 static, one workgroup per CU, 16 BUILD candidates and 48 (h, i) pairs per lane.
    # With 600 small tasks around it the grid (one workgroup per CU) is smaller than the batch: the workgroup that takes the large task has
    # had a small one before it and gets another one after it.
    d = cases.large_matrix("real4096")
    want = cases.large_want("real4096", 4096, k)
    big = large_task("real4096", 4096, k)
    got, ms = subpopr.pam_tasks(ctx, d, [big])
    print("4096 members, k = %d: %.1f ms in the kernel, %d swaps" % (k, ms, got[0]["n_swaps"]))
    assert same(got[0], want), (k, got[0]["medoids"], got[0]["n_swaps"])
    assert k == 1 or got[0]["n_swaps"] > 0                         # SWAP did run at the cap
    rng = np.random.default_rng(40 + k)
    pool = [(rng.choice(4096, size=m, replace=False).astype(np.int32), kk) for m, kk in ((2, 1), (3, 2), (5, 2), (9, 3), (17, 4), (33, 5), (64, 2), (65, 7))]
    tasks = [pool[i] for i in rng.integers(0, len(pool), size=600)]
    tasks.insert(300, big)
    got, ms = subpopr.pam_tasks(ctx, d, tasks)
    print("the same among 600 small tasks: %.1f ms" % ms)
    assert len(got) == 601
    for i, (t, g) in enumerate(zip(tasks, got)):
        assert same(g, want if i == 300 else want_of("real4096", d, t)), (i, len(t[0]), t[1])


def test_more_samples_than_the_cap_are_refused(ctx):
    d = np.zeros((4097, 4097))
    with pytest.raises(MsnvError) as err:
        subpopr.pam_tasks(ctx, d, [(np.arange(6, dtype=np.int32), 2)])
    assert err.value.code == EDOMAIN and "4097 samples (2 to 4096)" in str(err.value)
    with pytest.raises(MsnvError) as err:
        subpopr.prediction_strength(ctx, d, 2, np.arange(4097, dtype=np.int32).reshape(1, 1, 4097))
    assert err.value.code == EDOMAIN and "4097 samples (2 to 4096)" in str(err.value)


@pytest.mark.parametrize("n,k_max,big_m", [(513, 4, 2), (601, 4, 2), (3513, 3, 1)])
def test_prediction_strength_with_long_halves(ctx, n, k_max, big_m):
    # halves of 256 / 257 and 300 / 301: the tail kernel's loops over a split's entries make a second and a third trip (256 lanes); halves of
    # 1756 / 1757: the PAM launch of the splits raises its LDS limit
    d = cases.planted_dist_blocks(n, 3, 30 + n, noise=20.0)
    rng = np.random.default_rng(n)
    perms = np.array([[rng.permutation(n) for _ in range(big_m)] for _ in range(2, k_max + 1)], dtype=np.int32)
    got = subpopr.prediction_strength(ctx, d, k_max, perms, cutoff=0.8)
    prederr, mean_pred, optimalk = model.pred_strength(d, k_max, perms.tolist(), 0.8)
    print("n=%d: prederr %s mean.pred %s, %.1f ms in the kernels" % (n, prederr.tolist(), mean_pred, got["ms_kernel"]))
    assert got["prederr"].tobytes() == prederr.tobytes()
    assert got["mean_pred"].tobytes() == mean_pred.tobytes() and got["optimalk"] == optimalk
    assert 0.0 < prederr.min() and prederr.max() <= 1.0            # no empty or single-member cluster hides the pair counts


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


def outlier_case():
    names = cases.sample_names(45)
    table = cases.planted_freqs(45, 2, 8)
    table[40:44, ::3] = 45.0                                       # four samples with a third of their SNVs mixed: below 0.8 at 10 / 90
    table[44] = 100.0 - table[44]                                  # one sample unlike every other: the outlier
    table[3, 5] = np.nan                                           # a position without coverage does not count
    order = list(np.random.default_rng(1).permutation(45))         # the freq table lists the samples in another order
    return names, table, order


def test_stage_with_a_frequency_table_and_an_outlier(ctx, tmp_path):
    names, table, order = outlier_case()
    res, got = run_stage(ctx, tmp_path, names, cases.manhattan(np.nan_to_num(table, nan=0.0)), freq=([names[i] for i in order], table[order].T))
    assert res["n_outliers"] == 1 and res["n_samples"] == 40 and res["status"] == CLUSTER_OK and res["n_clusters"] == 2
    comp = got["sp_freq_composition.tab"].splitlines()
    assert comp[0] == "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95" and len(comp) == 46
    assert names[44] not in got["sp_mann_clustering.tab"] and names[41] not in got["sp_mann_clustering.tab"]


def test_stage_sums_the_frequency_counts_of_two_block_rows(ctx, tmp_path):
    # the same samples over 513 positions (the 60 rows repeated): a second block row of one position, and the >= 0.8 decision of every sample
    # taken on counts that atomics added up across the two
    names, table, order = outlier_case()
    long = table[:, np.arange(513) % 60]
    res, got = run_stage(ctx, tmp_path, names, cases.manhattan(np.nan_to_num(table, nan=0.0)), freq=([names[i] for i in order], long[order].T))
    assert res["n_outliers"] == 1 and res["n_samples"] == 40 and res["status"] == CLUSTER_OK and res["n_clusters"] == 2
    assert len(got["sp_freq_composition.tab"].splitlines()) == 46
    assert names[44] not in got["sp_mann_clustering.tab"] and names[41] not in got["sp_mann_clustering.tab"]


@pytest.mark.parametrize("s,n_pos", [(255, 511), (256, 512), (257, 513), (600, 1100), (257, 0)])
def test_frequency_composition_at_the_edges_of_its_grid(ctx, tmp_path, s, n_pos):
    # msnv_freq_bands_k: blocks of 256 sample columns by block rows of 512 positions.  One block short of a column and a position; exactly one;
    # a second block of one column and a second block row of one position; three ragged blocks by three block rows; a header-only table, for
    # which nothing is launched.  Five samples in the distance matrix, so the stage ends behind the kernel (fewer than 6 can pass).
    names = ["d%d.bam" % i for i in range(5)]
    fnames = cases.sample_names(s)
    for name, col in zip(names, (0, 255, 256, 257, s - 1)):        # the matrix's samples on the blocks' first and last columns, where those exist
        if col < s and fnames[col].startswith("s"):
            fnames[col] = name
    table = cases.band_table(n_pos, s, 50 + s)
    res, got = run_stage(ctx, tmp_path, names, cases.planted_dist(5, 0, 3), freq=(fnames, table))
    assert res["status"] == CLUSTER_TOO_FEW and sorted(got) == ["clustMedoidDefnFailed/sp_freq_composition.tab"]
    rows = [r.split("\t") for r in got["clustMedoidDefnFailed/sp_freq_composition.tab"].splitlines()[1:]]
    assert [r[0] for r in rows] == fnames
    nan = cases.band_nan_column(s)
    for c, r in enumerate(rows):
        assert (r[1:] == ["NaN"] * 3) == (c == nan or n_pos == 0), r   # 0 / 0 where no cell counts, a number everywhere else


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
