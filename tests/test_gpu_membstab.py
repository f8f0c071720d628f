"""The stability of each cluster's membership on the device (msnv_cluster_boot, msnv_membership_stability_file: csrc/cluster_k.hip, csrc/cluster.cpp)
against tests/membstabmodel.py, and subpopr.summarise_clustering on what the stages wrote.  Every comparison is exact: integers equal, files
byte-equal.

msnv_boot_match_k has one route: a workgroup of 256 lanes per subset, the k x k table in LDS.  The subset sizes are those where its entry loop and
the PAM kernel's loops change shape: 2 and 3 (the smallest), 63 / 64 / 65 (a wavefront), 255 / 256 / 257 (the workgroup: one entry per lane, then
two for lane 0), each with k = 1, 2, 15 and 32 where k < size.  The "dups" matrix has 10 distinct points, so at k = 15 and 32 medoids are
duplicates of each other and new clusters stay empty.  One call has 1756 members (the PAM launch before the matching raises its LDS limit above
48 KiB) and subsets of 1755, 900, 257 and 4 entries."""
import ctypes as C
import os

import numpy as np
import pytest

import membstabmodel as model
import pamcases as cases
import pammodel as pm
from metasnv_amd import core, subpopr
from metasnv_amd import _lib
from metasnv_amd._lib import MsnvError, EDOMAIN, EINVAL

pytestmark = pytest.mark.gpu
N, M = 264, 260
SIZES = (2, 3, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def matrix(kind):
    if kind == "planted":
        return cases.planted_dist(N, 4, 21, noise=30.0)
    return cases.integer_dist(N, 22) if kind == "integer" else cases.integer_dist(N, 23, distinct=10)


def members_of(seed):
    return np.sort(np.random.default_rng(seed).choice(N, size=M, replace=False)).astype(np.int32)


def same(got, want):
    clus, med, pairs = want
    return got["cluster"].tolist() == clus.tolist() and got["medoids"].tolist() == med.tolist() and got["pairs"].tolist() == pairs.tolist()


@pytest.mark.parametrize("k", [1, 2, 15, 32])
@pytest.mark.parametrize("kind", ["planted", "integer", "dups"])
def test_cluster_boot_at_every_size(ctx, kind, k):
    d = matrix(kind)
    members = members_of(3)
    rng = np.random.default_rng(100 + k)
    sets = [rng.choice(M, size=s, replace=False).astype(np.int32) for s in SIZES if s > k]
    got = subpopr.cluster_boot(ctx, d, members, k, sets)
    want = model.cluster_boot(d, members, k, sets)
    assert got["ms_kernel"] > 0 and got["pairs"].shape == (len(sets), k, 2)
    assert same(got, want), (kind, k)
    assert (got["pairs"][:, :, 1] > 0).all()                         # a union is never 0
    if kind == "dups" and k >= 15:                                   # medoids that are duplicates: clusters without a member were passed over
        assert len(set(got["cluster"].tolist())) < k
    if kind == "planted" and k == 32:                                # not every cluster is found again whole
        assert (got["pairs"][:, :, 0] > 0).any() and (got["pairs"][:, :, 0] != got["pairs"][:, :, 1]).any()


@pytest.mark.parametrize("kind", ["planted", "integer"])
def test_a_batch_larger_than_the_grid_gives_each_set_its_own_result(ctx, kind):
    d = matrix(kind)[:48, :48]
    members = np.arange(3, 43, dtype=np.int32)
    rng = np.random.default_rng(8)
    pool = [rng.choice(40, size=s, replace=False).astype(np.int32) for s in (4, 5, 7, 9, 12, 17, 23, 31, 40)]
    order = rng.integers(0, len(pool), size=4400)                    # 2048 workgroups at the most are resident (256 CUs x 8)
    order[0] = order[-1] = 5                                         # the same set first and last
    sets = [pool[i] for i in order]
    got = subpopr.cluster_boot(ctx, d, members, 3, sets)
    clus, med, pairs = model.cluster_boot(d, members, 3, pool)
    assert got["cluster"].tolist() == clus.tolist() and got["medoids"].tolist() == med.tolist()
    assert got["pairs"].tolist() == pairs[order].tolist()
    assert got["pairs"][0].tolist() == got["pairs"][-1].tolist()


@pytest.mark.parametrize("kind", ["real1756", "integer1756"])
def test_cluster_boot_on_a_long_list(ctx, kind):
    # 1756 members: the PAM launch raises its LDS limit (28 bytes per member, 49 168), the subsets of 1755, 900, 257 and 4 entries share it, and
    # the matching kernel's entry loop makes up to seven trips
    d = cases.large_matrix(kind)
    members = np.arange(1756, dtype=np.int32)
    rng = np.random.default_rng(17)
    sets = [rng.choice(1756, size=s, replace=False).astype(np.int32) for s in (1755, 900, 257, 4)]
    got = subpopr.cluster_boot(ctx, d, members, 3, sets)
    want = model.cluster_boot(d, members, 3, sets)
    print("%s: %.1f ms in the kernels, pairs %s" % (kind, got["ms_kernel"], got["pairs"].tolist()))
    assert got["pairs"].shape == (4, 3, 2) and same(got, want), kind
    assert (got["pairs"][:, :, 1] > 0).all() and sorted(set(got["cluster"].tolist())) == [1, 2, 3]


def test_the_whole_list_in_another_order_and_a_set_without_a_cluster(ctx):
    d = cases.planted_dist(72, 3, 5)
    members = np.arange(1, 71, dtype=np.int32)
    clus, _, _ = model.cluster_boot(d, members, 3, [])
    assert sorted(set(clus.tolist())) == [1, 2, 3]
    rng = np.random.default_rng(2)
    whole = rng.permutation(70).astype(np.int32)
    without3 = rng.permutation(np.flatnonzero(clus != 3)).astype(np.int32)
    sets = [whole, without3, np.arange(70, dtype=np.int32)]
    got = subpopr.cluster_boot(ctx, d, members, 3, sets)
    want = model.cluster_boot(d, members, 3, sets)
    assert same(got, want)
    assert got["pairs"][2].tolist() == [[s, s] for s in np.bincount(clus)[1:]]       # the list itself: every cluster found again
    assert got["pairs"][0].tolist() == got["pairs"][2].tolist()                      # far-apart groups: the order does not change the partition
    assert got["pairs"][1, 2, 0] == 0 and got["pairs"][1, 2, 1] > 0                  # cluster 3 has no entry in the set


# ---------------------------------------------------------------------------------- the stage on files
def write_used(path, names, d):
    """<species>_mann_distMatrixUsedForClustMedoidDefns.txt as the cluster stage writes it; returns the matrix a reader of it sees."""
    text = pm.dist_text(names, np.asarray(d), list(range(len(names))))
    with open(path, "w") as f:
        f.write(text)
    return np.array([[float(c) for c in ln.split("\t")[1:]] for ln in text.splitlines()[1:]])


NUM_STABILITY = "propSamples\tnumClusters\n" + "".join("%s\t3\n" % pm.fmt(0.8 + 0.1 * (i // 2)) for i in range(6))


def run_stage(ctx, tmp_path, d, k, num_text=None, **kw):
    names = cases.sample_names(d.shape[0])
    os.makedirs(str(tmp_path), exist_ok=True)
    used = str(tmp_path / "sp_mann_distMatrixUsedForClustMedoidDefns.txt")
    seen = write_used(used, names, d)
    num_path = None
    if num_text is not None:
        num_path = str(tmp_path / "sp_mann_clusNumStability.tab")
        with open(num_path, "w") as f:
            f.write(num_text)
    out = str(tmp_path / "out")
    res = subpopr.membership_stability_file(ctx, used, "sp", k, out, clus_num_stability_path=num_path, boot_iters=8, **kw)
    files, info = model.stability_files(seen, "sp", k, num_stability_text=num_text, seed=kw.get("seed", 1), boot_iters=8)
    got = {f: open(os.path.join(out, f)).read() for f in os.listdir(out)} if os.path.isdir(out) else {}
    assert sorted(got) == sorted(files)
    for f in files:
        assert got[f] == files[f], f
    for key in info:
        assert res[key] == info[key], key
    return res, got


def test_stage_three_planted_clusters_rate_high(ctx, tmp_path):
    res, got = run_stage(ctx, tmp_path, cases.planted_dist(120, 3, 1), 3, num_text=NUM_STABILITY)
    assert res["status"] == _lib.MEMBSTAB_OK and res["n_proportions"] == 8 and res["n_sets"] == 64 and res["ms_kernel"] > 0
    assert got["sp_mann_stabilityAssessment.tab"] == "name\tscore\nnumClusters\tHigh\nclust1\tHigh\nclust2\tHigh\nclust3\tHigh\n"
    rows = got["sp_mann_clusMembStability.tab"].splitlines()
    assert len(rows) == 1 + 8 * 3 and rows[1] == "1\t40\t0.3\t1\tInf"
    assert res["num_clusters_score"] == 3 and res["lowest_cluster_score"] == 3


def test_stage_without_structure_one_cluster(ctx, tmp_path):
    res, got = run_stage(ctx, tmp_path, cases.planted_dist(40, 0, 4), 1, seed=7)
    assert res["k"] == 1 and got["sp_mann_stabilityAssessment.tab"] == "name\tscore\nnumClusters\tNA\nclust1\tHigh\n"
    assert all(r.split("\t")[1:] == ["40", r.split("\t")[2], "1", "Inf"] for r in got["sp_mann_clusMembStability.tab"].splitlines()[1:])


def test_stage_twelve_samples_have_no_70_percent_row(ctx, tmp_path):
    res, got = run_stage(ctx, tmp_path, cases.planted_dist(12, 2, 1), 2)
    assert res["n_proportions"] == 2 and res["lowest_cluster_score"] == 0
    assert [r.split("\t")[2] for r in got["sp_mann_clusMembStability.tab"].splitlines()[1:]] == ["0.9", "0.9", "1", "1"]
    assert got["sp_mann_stabilityAssessment.tab"] == "name\tscore\nnumClusters\tNA\nclust1\tNA\nclust2\tNA\n"


def test_stage_nine_samples_are_not_rated(ctx, tmp_path):
    res, got = run_stage(ctx, tmp_path, cases.planted_dist(9, 2, 1), 2)
    assert res["status"] == _lib.MEMBSTAB_NOT_RATED and got == {} and not os.path.exists(str(tmp_path / "out"))


def test_stage_subsets_no_larger_than_k_give_rows_of_na(ctx, tmp_path):
    # 40 samples: the subsets of the first proportion have 12 entries, and pam cannot make 12 clusters of 12
    res, got = run_stage(ctx, tmp_path, cases.planted_dist(40, 4, 9, noise=30.0), 12)
    rows = [r.split("\t") for r in got["sp_mann_clusMembStability.tab"].splitlines()[1:]]
    assert res["n_proportions"] == 8 and res["n_sets"] == 7 * 8
    assert all(r[3:] == ["NA", "NA"] for r in rows[:12]) and all("NA" not in r for r in rows[12:])


def test_inputs_outside_the_domain_are_refused(ctx, tmp_path):
    d = cases.planted_dist(12, 2, 1)
    members = np.arange(12, dtype=np.int32)
    ok = np.arange(6, dtype=np.int32)
    for k, sets in ((6, [ok]), (7, [ok]), (2, [np.array([0, 1, 1, 2])]), (2, [np.array([0, 1, 12])]), (2, [np.array([0, -1, 3])]), (2, [np.arange(13) % 12]),
                    (0, [ok]), (12, []), (2, [ok, np.array([4, 5])])):
        with pytest.raises(MsnvError) as err:
            subpopr.cluster_boot(ctx, d, members, k, sets)
        assert err.value.code == EDOMAIN, (k, sets)
    big = cases.planted_dist(40, 0, 2)
    with pytest.raises(MsnvError) as err:                          # the table of one subset is 32 x 32
        subpopr.cluster_boot(ctx, big, np.arange(40, dtype=np.int32), 33, [np.arange(40, dtype=np.int32)])
    assert err.value.code == EDOMAIN
    with pytest.raises(MsnvError) as err:                          # members ascend
        subpopr.cluster_boot(ctx, d, members[::-1].copy(), 2, [ok])
    assert err.value.code == EDOMAIN
    e = d.copy()
    e[2, 7] += 1.0
    with pytest.raises(MsnvError) as err:
        subpopr.cluster_boot(ctx, e, members, 2, [ok])
    assert err.value.code == EDOMAIN
    used = str(tmp_path / "sp_mann_distMatrixUsedForClustMedoidDefns.txt")
    write_used(used, cases.sample_names(12), d)
    out = str(tmp_path / "out")
    for k in (0, 12, 33):
        with pytest.raises(MsnvError) as err:
            subpopr.membership_stability_file(ctx, used, "sp", k, out)
        assert err.value.code == EDOMAIN, k
    for boot in (0, 1025):
        with pytest.raises(MsnvError) as err:
            subpopr.membership_stability_file(ctx, used, "sp", 2, out, boot_iters=boot)
        assert err.value.code == EINVAL, boot
    o = _lib.MembStabOpts()
    _lib.lib.msnv_membstab_opts_default(C.byref(o))
    assert (o.seed, o.boot_iters, o.reserved) == (1, 100, 0)
    o.reserved = 1
    rc = _lib.lib.msnv_membership_stability_file(ctx._h, used.encode(), None, b"sp", 2, out.encode(), C.byref(o), (C.c_int64 * 8)(), None)
    assert rc == EINVAL and b"reserved" in _lib.lib.msnv_last_error()
    assert not os.path.exists(out)


def test_end_to_end_cluster_rate_summarise(ctx, tmp_path):
    names = cases.sample_names(60)
    dist_path = str(tmp_path / "sp.filtered.mann.dist")
    cases.write_dist(dist_path, names, cases.planted_dist(60, 2, 2))
    out = str(tmp_path / "out")
    res = subpopr.cluster_file(ctx, dist_path, out, stability_iters=2)
    assert res["status"] == _lib.CLUSTER_OK and res["optimalk"] == 2
    k = subpopr.clusters_from_ps_values(out, "sp")
    assert k == 2
    prefix = os.path.join(out, "sp_mann")
    rated = subpopr.membership_stability_file(ctx, prefix + "_distMatrixUsedForClustMedoidDefns.txt", "sp", k, out,
                                              clus_num_stability_path=prefix + "_clusNumStability.tab", boot_iters=8)
    assert rated["status"] == _lib.MEMBSTAB_OK and rated["num_clusters_score"] == res["stability_score"]
    # the model on what the cluster stage wrote
    files = {f: open(os.path.join(out, f)).read() for f in os.listdir(out) if os.path.isfile(os.path.join(out, f))}
    seen = np.array([[float(c) for c in ln.split("\t")[1:]] for ln in files["sp_mann_distMatrixUsedForClustMedoidDefns.txt"].splitlines()[1:]])
    want, _ = model.stability_files(seen, "sp", k, num_stability_text=files["sp_mann_clusNumStability.tab"], boot_iters=8)
    for f in want:
        assert files.pop(f) == want[f], f
    rows = subpopr.summarise_clustering(out)
    files.update(want)
    csv = open(os.path.join(out, "summary_clustering.csv")).read()
    assert csv == model.summary_csv(files)
    assert len(rows) == 1 and csv.splitlines()[1].startswith('"sp","sp",NA,60,2,') and csv.splitlines()[1].endswith(',"High-High","30-30","./sp_detailedSpeciesReport.html"')
