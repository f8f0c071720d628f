"""subpopr's genotyping positions on the device (csrc/genotype_k.hip, csrc/genotype.cpp) against tests/genotypemodel.py.  Every comparison is
exact: masks equal to the model's, files byte-equal.

msnv_genotype_rows_k has one route: a wavefront per table row, per cluster a lane-strided loop over the cluster's segment of the column list
and a butterfly over the 64 lanes.  The sizes are those where its loops change shape: 6 samples (a segment inside one wavefront), 63 / 64 / 65
and 129 / 300 (segments that end on, before and after a wavefront's width, several trips per lane) with 2, 3, 15 and 32 clusters (32: every
mask bit in use), one row, and more rows than the grid holds wavefronts (2048 workgroups of 4: device.h GENO_GRID_BLOCKS, GENO_ROWS_PER_BLOCK),
so that every wavefront takes a second trip."""
import glob
import os

import numpy as np
import pytest

import genotypecases as cases
import genotypemodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EFORMAT, GENOTYPE_OK, GENOTYPE_SINGLE, GENOTYPE_NO_POSITIONS, GENOTYPE_CLUSTER_MISSING, GENOTYPE_CUTOFF_BAD

pytestmark = pytest.mark.gpu
GRID_ROWS = 2048 * 4


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def check_rows(ctx, table, clust, threshold=80.0):
    got = subpopr.genotype_rows(ctx, table, clust, threshold)
    select, flip, near = model.genotype_rows(table, clust, threshold)
    assert got["select"].dtype == np.uint32 and got["select"].tolist() == select.tolist()
    assert got["flip"].tolist() == flip.tolist()
    return got, select, near


@pytest.mark.parametrize("s", [6, 63, 64, 65, 129, 300])
def test_masks_at_every_size(ctx, s):
    for k in (2, 3, 15, 32):
        if k > s:
            continue
        table, clust = cases.planted_genotypes(s, k, 8, 40, 100 * s + k, na_share=0.02)
        assert not model.genotype_rows(table, clust, guard=2e-6)[2].any()       # nothing within twice the kernel's guard ...
        got, select, _ = check_rows(ctx, table, clust)
        assert got["n_rechecked"] == 0, (s, k)                                  # ... so the kernel decides every row itself
        assert got["ms_kernel"] > 0
        if s >= 64:
            assert np.count_nonzero(select) > 4 * k
        if k == 32:
            assert int(np.bitwise_or.reduce(select)) == 0xffffffff and int(np.bitwise_or.reduce(got["flip"])) == 0xffffffff


def test_one_row(ctx):
    table, clust = cases.planted_genotypes(65, 3, 1, 0, 3)
    got, select, _ = check_rows(ctx, table[:1], clust)
    assert select.tolist() == [1]


def test_more_rows_than_the_grid_holds_wavefronts(ctx):
    table, clust = cases.planted_genotypes(6, 2, 8, GRID_ROWS + 5, 17)
    table = np.roll(table, -16, axis=0)                                        # the 16 planted rows last: rows of the second trip
    assert len(table) == GRID_ROWS + 21
    got, select, near = check_rows(ctx, table, clust)
    assert select[GRID_ROWS + 5:].tolist() == [3] * 16 and got["flip"][GRID_ROWS + 5:].tolist() == [2, 1] * 4 + [1, 2] * 4
    assert got["n_rechecked"] == int(near.sum())


def test_columns_not_in_use(ctx):
    table, clust = cases.planted_genotypes(70, 3, 8, 40, 23, na_share=0.02)
    rng = np.random.default_rng(4)
    clust = clust.copy()
    clust[[0, 5, 33, 64, 69]] = 0
    table[:, [0, 5, 33, 64, 69]] = rng.uniform(0, 100, size=(len(table), 5)).round(3)      # what they hold must not matter
    table[::3, 33] = np.nan
    got, select, _ = check_rows(ctx, table, clust)
    assert np.count_nonzero(select) > 12


def test_rows_at_the_threshold_are_decided_by_the_long_double_rule(ctx):
    clust = np.array([1, 1, 1, 2, 2, 2, 2])
    inside = clust == 1
    rows = [np.where(inside, 90.0, 10.0)] * 20 + [np.where(inside, 10.0, 90.0)] * 20        # exactly 80: not selected
    rows += [np.where(inside, 90.5, 10.0)] * 20 + [np.where(inside, 10.0, 90.5)] * 20       # 80.5: selected, not near
    for a in np.arange(0.81, 1.0, 0.005):                                                  # products that miss their decimal by an ulp or two
        lo = round(a - 0.8, 3)
        rows += [np.where(inside, a * 100, lo * 100), np.where(inside, lo * 100, a * 100)]
        rows.append(np.array([a * 100, (a + 0.001) * 100, (a - 0.001) * 100, lo * 100, lo * 100, (lo + 0.002) * 100, max(lo - 0.002, 0) * 100]))
    table = np.array(rows, dtype=np.float64)
    got, select, near = check_rows(ctx, table, clust)
    assert select[:40].tolist() == [0] * 40 and select[40:80].tolist() == [3] * 40
    assert got["n_rechecked"] >= 80 and got["n_rechecked"] == int(near.sum()) and not near[40:80].any()
    assert 0 < np.count_nonzero(select[80:]) < len(select) - 80                             # the long double rule falls on both sides


def test_inputs_outside_the_domain_are_refused(ctx):
    table, clust = cases.planted_genotypes(12, 2, 4, 4, 1)
    for bad in (100.5, -0.001, np.inf):
        t = table.copy()
        t[5, 7] = bad
        with pytest.raises(MsnvError) as err:
            subpopr.genotype_rows(ctx, t, clust)
        assert err.value.code == EDOMAIN, bad
    for c in ([1] * 12, [1] * 6 + [3] * 6, [1] * 11 + [33]):                    # one cluster, a cluster without a column, 33 clusters
        with pytest.raises(MsnvError) as err:
            subpopr.genotype_rows(ctx, table, np.array(c))
        assert err.value.code == EDOMAIN, c


# ---------------------------------------------------------------------------------------------- the stage
def read_tree(root):
    out = {}
    for dp, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p).read()
    return out


def run_stage(ctx, tmp_path, clustering, names, table01, **kw):
    os.makedirs(str(tmp_path), exist_ok=True)
    labels = cases.row_labels(len(table01))
    clust_path, freq_path, out = str(tmp_path / "sp_mann_clustering.tab"), str(tmp_path / "sp.filtered.freq"), str(tmp_path / "out")
    open(clust_path, "w").write(clustering)
    cases.write_freq(freq_path, names, labels, table01)
    files, info = model.genotype_files(clustering, (names, labels, table01), "sp", **kw)
    res = subpopr.genotype_file(ctx, clust_path, freq_path, out, **kw)
    got = read_tree(out)
    assert sorted(got) == sorted(files)
    for f in files:
        assert got[f] == files[f], f
    for key in ("status", "n_clusters", "n_samples", "n_rows", "n_positions", "n_correct", "n_good"):
        assert res[key] == info[key], key
    return res, got


def planted_stage(seed, n=120, k=3, background=40):
    table, clust = cases.planted_genotypes(n, k, 8, background, seed, na_share=0.02)
    return (table / 100.0).round(5), clust, cases.sample_names(n)


def test_stage_three_planted_clusters(ctx, tmp_path):
    table, clust, names = planted_stage(31)
    order = np.random.default_rng(1).permutation(120)                              # the clustering file lists the samples in another order
    clustering = model.clustering_text((names[i], int(clust[i]) + 3) for i in order if i not in (7, 50))       # two freq columns are not in use
    res, got = run_stage(ctx, tmp_path, clustering, names, table)
    assert res["status"] == GENOTYPE_OK and res["n_clusters"] == 3 and res["n_samples"] == 118 and res["n_positions"] >= 18
    assert res["n_good"] == 118 and res["n_correct"] == 0                          # ids 4, 5, 6 never equal a column index: the reference's comparison
    assert sorted(got) == ["sp_4_hap_positions.tab", "sp_5_hap_positions.tab", "sp_6_hap_positions.tab", "sp_hap_freq_mean.tab", "sp_hap_freq_median.tab", "sp_hap_out.txt"]
    assert len(got["sp_hap_freq_median.tab"].splitlines()) == 1 + 3 * 118
    clustering = model.clustering_text((names[i], int(clust[i])) for i in order)
    res, _ = run_stage(ctx, tmp_path / "ids123", clustering, names, table)
    assert res["status"] == GENOTYPE_OK and res["n_correct"] == 120 and res["ms_kernel"] > 0


def test_stage_single_cluster(ctx, tmp_path):
    table, clust, names = planted_stage(32, n=12, k=2, background=4)
    res, got = run_stage(ctx, tmp_path, model.clustering_text((n, 1) for n in names), names, table)
    assert res["status"] == GENOTYPE_SINGLE and got == {"sp_hap_out.txt": "Single cluster\n"} and res["ms_kernel"] == 0


def test_stage_no_positions(ctx, tmp_path):
    table, clust, names = planted_stage(33, n=30, k=3)
    res, got = run_stage(ctx, tmp_path, model.clustering_text(zip(names, clust.tolist())), names, table[24:])       # the background rows only
    assert res["status"] == GENOTYPE_NO_POSITIONS and sorted(got) == ["sp_hap_out.txt"] and got["sp_hap_out.txt"].endswith("No genotyping positions for  sp\n")


def test_stage_one_cluster_missing(ctx, tmp_path):
    table, clust, names = planted_stage(34, n=60, k=3)
    res, got = run_stage(ctx, tmp_path, model.clustering_text(zip(names, clust.tolist())), names, np.concatenate([table[:16], table[24:]]))
    assert res["status"] == GENOTYPE_CLUSTER_MISSING and sorted(got) == ["sp_1_hap_positions.tab", "sp_2_hap_positions.tab", "sp_hap_out.txt"]


def test_stage_cutoff_bad(ctx, tmp_path):
    table, clust, names = planted_stage(35)
    table[:, :19] = np.where(np.isnan(table[:, :19]), np.nan, 0.5)                 # 19 of 120 samples mixed at 50: each sums to 150 over three clusters
    res, got = run_stage(ctx, tmp_path, model.clustering_text(zip(names, clust.tolist())), names, table, uniq_threshold=0.7)
    assert res["status"] == GENOTYPE_CUTOFF_BAD and "In  19  out of  120  samples" in got["sp_hap_out.txt"] and "sp_hap_freq_mean.tab" not in got


def test_stage_refuses_old_style_tables_and_broken_clusterings(ctx, tmp_path):
    table, clust, names = planted_stage(36, n=12, k=2, background=4)
    table[3, 4] = 1.5
    with pytest.raises(model.DomainError):
        model.genotype_files(model.clustering_text(zip(names, clust.tolist())), (names, cases.row_labels(len(table)), table), "sp")
    clust_path, freq_path = str(tmp_path / "c.tab"), str(tmp_path / "sp.filtered.freq")
    open(clust_path, "w").write(model.clustering_text(zip(names, clust.tolist())))
    cases.write_freq(freq_path, names, cases.row_labels(len(table)), table)
    with pytest.raises(MsnvError) as err:
        subpopr.genotype_file(ctx, clust_path, freq_path, str(tmp_path / "out"))
    assert err.value.code == EDOMAIN and not os.path.exists(str(tmp_path / "out"))
    table[3, 4] = 0.5
    cases.write_freq(freq_path, names, cases.row_labels(len(table)), table)
    open(clust_path, "w").write(model.clustering_text(zip(names, ["NA"] + clust.tolist()[1:])))
    with pytest.raises(MsnvError) as err:
        subpopr.genotype_file(ctx, clust_path, freq_path, str(tmp_path / "out"))
    assert err.value.code == EFORMAT


def test_positions_feed_the_genotyping_subset(ctx, tmp_path, golden_dir):
    """The chain: this stage's *_hap_positions.tab are what getGenotypingSNVSubset.py reads."""
    snps = os.path.join(golden_dir, "subpopr", "one", "metasnv", "snpCaller", "called_SNPs")
    lines = open(snps).read().splitlines(True)[:24]
    labels = []
    for ln in lines:
        f = ln.split("\t")
        labels.append("%s:%s:%s:%s:." % (f[0], f[1], f[2], f[5].split("|")[1]))
    assert len({(ln.split("\t")[0], ln.split("\t")[2]) for ln in lines}) == 24
    names = list("abcdef")
    table = np.full((24, 6), 0.5)
    table[0:5] = [1, 1, 1, 0, 0, 0]                                               # rows 0-4 genotype both clusters ...
    table[5:8] = [0, 0, 0.02, 1, 0.97, 1]
    table[8] = [1, 1, -1, 0, 0, 0]                                                # ... row 8 neither: a sample without coverage
    table[table < 0] = np.nan
    hap = tmp_path / "hap"
    clust_path, freq_path = str(tmp_path / "spA_mann_clustering.tab"), str(tmp_path / "spA.filtered.freq")
    open(clust_path, "w").write(model.clustering_text(zip(names, [1, 1, 1, 2, 2, 2])))
    cases.write_freq(freq_path, names, labels, table)
    res = subpopr.genotype_file(ctx, clust_path, freq_path, str(hap))
    assert res["status"] == GENOTYPE_OK and res["n_positions"] == 16
    haps = sorted(glob.glob(str(hap / "*hap_positions.tab")))
    assert [os.path.basename(h) for h in haps] == ["spA_1_hap_positions.tab", "spA_2_hap_positions.tab"]
    n_pos, n_lines = subpopr.genotyping_subset(haps, [snps], str(hap))
    assert n_pos == 8 and n_lines >= 16
    wanted = {(ln.split("\t")[0], ln.split("\t")[2]) for ln in lines[:8]}
    want = "".join(ln for ln in open(snps).read().splitlines(True) if (ln.split("\t")[0], ln.split("\t")[2]) in wanted)
    for c in (1, 2):
        assert open(str(hap / ("spA_%d.pos" % c))).read() == want
