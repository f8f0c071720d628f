"""subpopr's subspecies profile on the device (csrc/profile_k.hip, csrc/profile.cpp) against tests/profilemodel.py.  Every comparison is exact: integers
equal, doubles equal as bit patterns, files byte-equal.

msnv_profile_columns_k has one route: a workgroup of 16 wavefronts per 16 columns, a lane per (column, sub-row), 64 rows per step and four steps in
flight, eight radix passes.  The sizes are those where its loops change shape: 1 and 2 columns (a band almost empty), 63 / 64 / 65 and 130 / 300 (a
last workgroup that is full, one short and one over; several workgroups) with 1, 2, 3 rows (fewer rows than sub-rows), 64 / 65 (one step, and one row
over) and 1000 (several unrolled trips, a ragged last one); 5000 rows by 6 columns is the single workgroup whose wavefronts split the rows."""
import os

import numpy as np
import pytest

import genotypecases
import genotypemodel
import profilecases as cases
import profilemodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EFORMAT, PROFILE_OK, PROFILE_NO_FILES, PROFILE_NONE_USABLE, GENOTYPE_OK

pytestmark = pytest.mark.gpu
INTS = ("n_called", "n_gt0", "n_ge5", "n_eq0", "n_eq100")
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def check_columns(ctx, rows, flip, cols_per_pass=0):
    got = subpopr.profile_columns(ctx, rows, flip, cols_per_pass)
    want = model.profile_columns(rows, flip)
    for k in INTS:
        assert got[k].dtype == np.uint32 and got[k].tolist() == want[k].tolist(), k
    for k in ("mid_lo", "mid_hi"):
        g, w = got[k], want[k]
        assert np.isnan(g).tolist() == np.isnan(w).tolist(), k
        assert g[~np.isnan(g)].view(np.uint64).tolist() == w[~np.isnan(w)].view(np.uint64).tolist(), k
    return got


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 130, 300])
def test_columns_at_every_size(ctx, s):
    for g in (1, 2, 3, 64, 65, 1000):
        for mix in cases.MIXES:
            rows = cases.matrix(mix, g, s, 7)
            got = check_columns(ctx, rows, np.zeros(g, dtype=bool))
            assert got["ms_kernel"] > 0
            if mix == "nan_column":
                assert got["n_called"][-1] == 0 and np.isnan(got["mid_lo"][-1])
            if mix == "two_called" and g > 1:
                assert got["n_called"][-1] == 2 and (got["mid_lo"][-1], got["mid_hi"][-1]) == (12.25, 100.0)


def test_few_columns_many_rows(ctx):
    for mix in cases.MIXES:
        check_columns(ctx, cases.matrix(mix, 5000, 6, 8), cases.flips(5000, 8))


@pytest.mark.parametrize("s", [2, 65, 130])
def test_half_the_rows_flipped(ctx, s):
    for g in (3, 65, 1000):
        for mix in ("real", "low_bits", "neg_zero", "two_called"):
            rows, flip = cases.matrix(mix, g, s, 9), cases.flips(g, 9)
            got = check_columns(ctx, rows, flip)
            if mix == "real" and g == 1000:                             # the flips are seen: not the statistics of the matrix as it stands
                assert got["n_eq0"].tolist() != model.profile_columns(rows, np.zeros(g, dtype=bool))["n_eq0"].tolist()


def test_column_bands(ctx):
    rows, flip = cases.matrix("real", 200, 130, 10), cases.flips(200, 10)
    rows[:, 64] = cases.matrix("low_bits", 200, 1, 10)[:, 0]            # the first column of the second band of 64
    whole = check_columns(ctx, rows, flip)
    for width in (64, 50, 130, 1000):                                   # three bands, three ragged ones, one, one wider than the matrix
        got = check_columns(ctx, rows, flip, cols_per_pass=width)
        for k in INTS + ("mid_lo", "mid_hi"):
            assert got[k].tobytes() == whole[k].tobytes(), (width, k)


def test_inputs_outside_the_domain_are_refused(ctx):
    rows = cases.matrix("real", 70, 20, 11)
    for bad, flipped in ((100.5, False), (-1.0, False), (np.inf, False), (-0.5, True), (100.5, True)):
        t = rows.copy()
        t[33, 17] = bad
        flip = np.zeros(70, dtype=bool)
        flip[33] = flipped
        with pytest.raises(MsnvError) as err:
            subpopr.profile_columns(ctx, t, flip)
        assert err.value.code == EDOMAIN, bad
    for shape in ((5, 0), (0, 5)):                                      # n_samples = 0, n_rows = 0
        with pytest.raises(MsnvError) as err:
            subpopr.profile_columns(ctx, np.zeros(shape), np.zeros(shape[0], dtype=bool))
        assert err.value.code == EDOMAIN, shape


# ---------------------------------------------------------------------------------------------- the stage
def write_tree(root, tree):
    os.makedirs(str(root), exist_ok=True)
    for name, text in tree.items():
        open(str(root / name), "w").write(text)


def run_stage(ctx, tmp_path, tree, samples, **kw):
    out = tmp_path / "out"
    write_tree(out, tree)
    open(str(tmp_path / "all_samples"), "w").write(samples)
    stat = out / "sp_extended_clustering_stat.txt"
    open(str(stat), "w").write("an earlier line\n")                     # the stage appends
    try:
        files, info = model.profile_files("sp", samples, tree, **kw)
        error = None
    except model.DomainError as e:
        files, info, error = e.files, None, e
    try:
        res = subpopr.subpop_profile_files(ctx, "sp", str(out), str(tmp_path / "all_samples"), **kw)
        assert error is None
    except MsnvError as e:
        assert error is not None and e.code == EDOMAIN
        res = e
    got = {f: open(str(out / f)).read() for f in os.listdir(str(out)) if f not in tree}
    assert got.pop(stat.name) == "an earlier line\n" + files.get(stat.name, "")
    assert sorted(got) == sorted(f for f in files if f != stat.name)
    for f in got:
        assert got[f] == files[f], f
    if info is not None:
        for key in info:
            assert res[key] == info[key], key
    return res, got


def test_stage_three_planted_clusters(ctx, tmp_path):
    tree, samples, truth = cases.planted_project()
    res, got = run_stage(ctx, tmp_path, tree, samples)
    assert res["status"] == PROFILE_OK and (res["n_usable"], res["n_full"], res["n_filtered"], res["n_incoherent"], res["n_bad"]) == (3, 39, 36, 2, 1)
    assert res["ms_kernel"] > 0 and len(got) == 4
    res, got = run_stage(ctx, tmp_path / "strict", tree, samples, max_prop_uncalled=0.9, min_genotype_abundance=99.5)
    assert res["status"] == PROFILE_OK and res["n_full"] == 30 and res["n_assigned"] == 28


def test_stage_without_cluster_files(ctx, tmp_path):
    res, got = run_stage(ctx, tmp_path, {"sp_1.pos": "", "spx_1.pos.freq": ""}, "a\nb\n")
    assert res["status"] == PROFILE_NO_FILES and got == {}


def test_stage_no_cluster_usable(ctx, tmp_path):
    none, full = [NAN] * 3, [100.0, 0.0, 100.0]
    tree = {}
    for c, cols in ((1, [none, none, full]), (2, [none, none, none])):
        tree["sp_%d.pos.freq" % c] = cases.freq_text(["k:-:%d:A" % p for p in range(3)], np.array(cols).T)
        tree["sp_%d_hap_positions.tab" % c] = cases.hap_text(["k:-:%d:T>A:." % p for p in range(3)], [False] * 3)
    res, got = run_stage(ctx, tmp_path, tree, "a\nb\nc\n")
    assert res["status"] == PROFILE_NONE_USABLE and res["n_files"] == 2 and got == {}


def test_stage_where_the_reference_breaks(ctx, tmp_path):
    none, full = [NAN] * 3, [100.0, 0.0, 100.0]

    def tree_of(by_cluster):
        tree = {}
        for c, cols in by_cluster.items():
            tree["sp_%d.pos.freq" % c] = cases.freq_text(["k:-:%d:A" % p for p in range(3)], np.array(cols).T)
            tree["sp_%d_hap_positions.tab" % c] = cases.hap_text(["k:-:%d:T>A:." % p for p in range(3)], [False, True, False])
        return tree
    err, got = run_stage(ctx, tmp_path / "a", tree_of({2: [full, full], 3: [full, full]}), "a\nb\n")
    assert isinstance(err, MsnvError) and "cluster 1 is not among the usable clusters" in str(err) and list(got) == ["sp_extended_clustering_abundanceSummaryStats.tsv"]
    err, got = run_stage(ctx, tmp_path / "b", tree_of({1: [full, full, none, none], 2: [none, none, full, full]}), "a\nb\nc\nd\n")
    assert isinstance(err, MsnvError) and "no sample has a median in every usable cluster" in str(err) and list(got) == ["sp_extended_clustering_abundanceSummaryStats.tsv"]


def test_stage_refuses_broken_inputs(ctx, tmp_path):
    tree, samples, _ = cases.planted_project(n_samples=10, sizes=(5, 5, 5))
    good = dict(tree)

    def refused(code, **kw):
        write_tree(tmp_path / "out", tree)
        open(str(tmp_path / "all_samples"), "w").write(samples)
        with pytest.raises(MsnvError) as err:
            subpopr.subpop_profile_files(ctx, "sp", str(tmp_path / "out"), str(tmp_path / "all_samples"), **kw)
        assert err.value.code == code
        return str(err.value)
    for bad in (0.0, 1.5):
        refused(EDOMAIN, max_prop_uncalled=bad)
    first = next(ln for ln in good["sp_1.pos.freq"].split("\n") if ln.startswith("ctg.1:gene1000:1000:A\t"))      # a listed position
    tree["sp_1.pos.freq"] = good["sp_1.pos.freq"] + first + "\n"                                   # a duplicate id
    assert "occurs twice" in refused(EFORMAT)
    tree["sp_1.pos.freq"] = good["sp_1.pos.freq"].replace(first, first + "\t5.0")                   # a column too many
    assert "does not have expected number of columns (each column is a sample). According to all_samples, it should have 10 columns." in refused(EFORMAT)
    tree["sp_1.pos.freq"] = good["sp_1.pos.freq"].replace(first, "\t".join([first.split("\t")[0]] + ["150.0"] * 10))
    refused(EDOMAIN)                                                                               # a cell outside [0, 100]
    tree["sp_1.pos.freq"] = good["sp_1.pos.freq"]
    tree["sp_x.pos.freq"] = good["sp_1.pos.freq"]
    assert "Species-cluster name did not conform to expectations." in refused(EFORMAT)
    os.remove(str(tmp_path / "out" / "sp_x.pos.freq"))
    del tree["sp_x.pos.freq"]
    hap = good["sp_2_hap_positions.tab"].split("\n")
    tree["sp_2_hap_positions.tab"] = "\n".join(hap[:3] + [hap[2]] + hap[3:])                        # a position listed twice
    assert "occurs twice" in refused(EFORMAT)


def test_chain_from_the_frequency_table_to_the_gene_content(ctx, tmp_path):
    """genotype_file -> genotyping_subset -> snv_allele_freq -> subpop_profile_files -> subpop_abundance_files -> gene_corr_files on a synthetic project
    of 12 samples and two planted subspecies: every stage reads its predecessor's files as written."""
    n, n_pos = 12, 16
    names = genotypecases.sample_names(n)
    truth = np.arange(n) % 2 + 1
    meta, out = tmp_path / "metasnv", tmp_path / "out"
    os.makedirs(str(meta / "snpCaller"))
    open(str(meta / "all_samples"), "w").write(cases.all_samples_text(names))
    rng = np.random.default_rng(5)
    high_in = np.arange(n_pos) % 2 + 1                                   # the subspecies that carries the alternative allele of position p
    table = np.where(truth[None, :] == high_in[:, None], 1.0, 0.0)
    table = np.concatenate([table, rng.uniform(0.3, 0.7, size=(6, n)).round(3)])      # six rows that tell nothing
    labels = ["ctg:-:%d:T>A:." % (10 * p + 7) for p in range(len(table))]
    with open(str(meta / "snpCaller" / "called_SNPs.best_split_1"), "w") as f:
        for p, row in enumerate(table):
            cov = rng.integers(20, 40, size=n)
            alt = np.rint(cov * row).astype(int)
            f.write("ctg\t-\t%d\tT\t%s\t%d|A|.|%s\n" % (10 * p + 7, "|".join(map(str, cov)), alt.sum(), "|".join(map(str, alt))))
    clust_path, freq_path = str(tmp_path / "sp_mann_clustering.tab"), str(tmp_path / "sp.filtered.freq")
    open(clust_path, "w").write(genotypemodel.clustering_text(zip(names, truth.tolist())))
    genotypecases.write_freq(freq_path, names, labels, table)
    res = subpopr.genotype_file(ctx, clust_path, freq_path, str(out))
    assert res["status"] == GENOTYPE_OK and res["n_positions"] == 2 * n_pos and os.path.exists(str(out / "sp_hap_freq_median.tab"))
    haps = sorted(str(out / f) for f in os.listdir(str(out)) if f.endswith("hap_positions.tab"))
    subpopr.genotyping_subset(haps, [str(meta / "snpCaller" / "called_SNPs.best_split_1")], str(out))
    for c in (1, 2):
        rows, _ = subpopr.snv_allele_freq(ctx, str(out / ("sp_%d.pos" % c)), 5)
        assert rows == n_pos
    res = subpopr.subpop_profile_files(ctx, "sp", str(out), str(meta / "all_samples"))
    assert res["status"] == PROFILE_OK and (res["n_usable"], res["n_full"], res["n_filtered"], res["n_assigned"]) == (2, n, n, n)
    clust = open(str(out / "sp_extended_clustering.tab")).read()
    assert clust == "clust\n" + "".join("%s\t%d\n" % (nm, t) for nm, t in zip(names, truth))
    abund = rng.uniform(0.01, 0.2, size=n).round(4)
    open(str(tmp_path / "species.tsv"), "w").write("\t" + "\t".join(names) + "\nsp\t" + "\t".join(repr(float(v)) for v in abund) + "\n")
    assert subpopr.subpop_abundance_files("sp", str(out), str(tmp_path / "species.tsv")) == (n, 2, n, n)
    rel = open(str(out / "sp_allClust_relativeAbund.tab")).read().split("\n")
    assert rel[0] == "X1\tX2" and rel[1] == "%s\t%s\t0" % (names[0], genotypemodel.fmt(100.0 / 100.0 * abund[0]))
    genes = rng.uniform(1, 50, size=(5, n)).round(3)
    genes[0] = np.where(truth == 1, abund * 1000, 0.001).round(6)        # a gene family that follows subspecies 1
    open(str(tmp_path / "genes.tsv"), "w").write("gene\t" + "\t".join(names) + "\n" + "".join(
        "g%d\t%s\n" % (i, "\t".join(repr(float(v)) for v in row)) for i, row in enumerate(genes)))
    k, g, s, _ = subpopr.gene_corr_files(ctx, str(out / "sp_allClust_relativeAbund.tab"), str(tmp_path / "genes.tsv"), str(out / "sp_corrGenes"))
    assert (k, g, s) == (2, 5, n)                                        # the reader takes the X1 / X2 headers
    assert os.path.getsize(str(out / "sp_corrGenes-spearman.tsv")) > 0
