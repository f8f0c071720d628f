"""subpopr's PCoA on the device (csrc/pcoa_k.hip, csrc/pcoa.cpp) against tests/pcoamodel.py.  Every comparison with the model is exact: doubles
bit-equal, integers equal, files byte-equal.

The sizes are those where the kernels' loops change shape.  msnv_pcoa_params_k has one lane per pair and 128 lanes per workgroup;
msnv_pcoa_rotate_k lays 64 column pairs along a wavefront and four row pairs (or rows of V) across a workgroup.  So: 2 (one pair, nothing but its
own block), 3 and 5 (odd: slot 0 is the bye, a block of one row), 4, 63 / 64 / 65 (31 or 32 pairs and a bye, 32 pairs, 32 pairs and a bye), and
127 .. 130 (63 pairs and a bye, 64 pairs: a whole wavefront, 64 and a bye, 65: a second workgroup column of one pair).  At 513 samples the 257
slots take three workgroups of the parameter kernel; the numpy model is too slow there, so the solve is checked by what an eigendecomposition
must satisfy, with the bounds of tests/test_pcoa_model.py, and against numpy.linalg.eigh."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pamcases
import pammodel
import pcoacases as cases
import pcoamodel as model
from metasnv_amd import core, subpopr
from metasnv_amd._lib import MsnvError, EDOMAIN, EINVAL, CLUSTER_OK, CLUSTER_NONE, PCOA_OK, PCOA_TOO_FEW_AXES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def same(got, want, n_axes):
    for key in ("eig", "rel_eig", "axis_pct"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["vectors"].tobytes() == np.ascontiguousarray(want["vectors"][:, :n_axes]).tobytes()
    for key in ("status", "sweeps", "rotations", "k", "n_negative"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("n", cases.GPU_SIZES)
@pytest.mark.parametrize("kind", ["manhattan", "integer"])
def test_pcoa_at_every_size(ctx, kind, n):
    d = cases.matrix(kind, n)
    want = cases.want(kind, n)
    for n_axes in sorted({min(2, n), n}):
        got = subpopr.pcoa(ctx, d, n_axes)
        print("%s n=%d axes=%d: %d sweeps, %d rotations, k=%d, %.2f ms in the kernels" % (kind, n, n_axes, got["sweeps"], got["rotations"], got["k"], got["ms_kernel"]))
        same(got, want, n_axes)
    assert n == 2 or want["rotations"] > 0
    if kind == "manhattan" and n >= 63:
        assert want["n_negative"] > 0                              # the branch real data takes (a handful of samples embed exactly)
    if kind == "integer" and n > 5:
        assert (d == 0).sum() > n and want["k"] < n - 1            # duplicated samples: eigenvalues the cut-off set to 0, NaN columns


def test_513_samples_across_three_workgroups_of_pairs(ctx):
    n = 513
    d = pamcases.planted_dist_blocks(n, 3, 613, noise=30.0)
    b, trace = model.centre(d)
    got = subpopr.pcoa(ctx, d, n)
    want = np.linalg.eigh(b)[0][::-1]
    top = np.abs(want).max()
    k = got["k"]
    lam = got["eig"]
    print("n=513: %d sweeps, %d rotations, k=%d, %d negative, %.1f ms in the kernels" % (got["sweeps"], got["rotations"], k, got["n_negative"], got["ms_kernel"]))
    assert got["status"] == PCOA_OK and got["sweeps"] <= 64 and (np.diff(lam) <= 0).all() and got["n_negative"] > 0
    cut = np.where(np.abs(want) < model.CUT, 0.0, want)
    err_eig = np.abs(lam - cut).max() / (EPS * top)
    assert k == int((want > model.CUT).sum()) and 2 < k < n and np.isnan(got["vectors"][:, k:]).all()
    v = got["vectors"][:, :k] / np.sqrt(lam[:k])[None, :]           # the eigenvectors of the k axes that have one
    err_res = np.abs(b @ v - v * lam[None, :k]).max() / (EPS * top)
    err_orth = np.abs(v.T @ v - np.eye(k)).max() / EPS
    print("eigenvalues %.2f, residual %.2f (x 2^-52 max |lambda|), orthogonality %.2f n 2^-52" % (err_eig, err_res, err_orth / n))
    assert err_eig <= 4 * n and err_res <= 4 * n and err_orth <= 4 * n
    top_rows = np.argmax(np.abs(got["vectors"][:, :k]), axis=0)
    assert (got["vectors"][top_rows, np.arange(k)] > 0).all()      # the sign rule
    assert np.abs(got["rel_eig"] - lam / trace).max() <= 4 * EPS and abs(got["axis_pct"].sum() - 100.0) <= n * EPS * 100


def test_a_solve_does_not_depend_on_its_place_in_the_process(ctx):
    d = cases.matrix("manhattan", 65)
    first = subpopr.pcoa(ctx, d, 65)
    subpopr.pcoa(ctx, cases.matrix("integer", 130), 2)
    again = subpopr.pcoa(ctx, d, 65)
    same(first, cases.want("manhattan", 65), 65)
    same(again, first, 65)


def test_inputs_outside_the_domain_are_refused(ctx):
    d = cases.matrix("manhattan", 8)
    for i, j, bad in ((2, 5, -1.0), (2, 5, np.nan), (2, 5, np.inf), (3, 3, 0.5)):
        e = d.copy()
        e[i, j] = e[j, i] = bad
        with pytest.raises(MsnvError) as err:
            subpopr.pcoa(ctx, e, 2)
        assert err.value.code == EDOMAIN, bad
    e = d.copy()
    e[2, 5] += 1.0                                                 # not symmetric
    with pytest.raises(MsnvError) as err:
        subpopr.pcoa(ctx, e, 2)
    assert err.value.code == EDOMAIN
    with pytest.raises(MsnvError) as err:
        subpopr.pcoa(ctx, np.zeros((1, 1)), 1)
    assert err.value.code == EDOMAIN
    for n_axes in (0, 9):
        with pytest.raises(MsnvError) as err:
            subpopr.pcoa(ctx, d, n_axes)
        assert err.value.code == EINVAL, n_axes


# ---------------------------------------------------------------------------------------------- the stage on files
def clustered(ctx, tmp_path, names, d, freq=None, **kw):
    """The inputs of the stage as clusterSubpops.py leaves them: (dist_path, out_dir, cluster_file's result)."""
    dist_path = str(tmp_path / "sp.filtered.mann.dist")
    pamcases.write_dist(dist_path, names, d)
    freq_path = None
    if freq is not None:
        freq_path = str(tmp_path / "sp.filtered.freq")
        pamcases.write_freq(freq_path, freq[0], freq[1])
    out = str(tmp_path / "out")
    return dist_path, out, subpopr.cluster_file(ctx, dist_path, out, freq_path=freq_path, stability_iters=2, **kw)


def model_files(names, d, directory):
    comp = os.path.join(directory, "sp_freq_composition.tab")
    return model.pcoa_files(names, d, "sp", open(os.path.join(directory, "sp_mann_clustering.tab")).read(), open(comp).read() if os.path.exists(comp) else None)


def check_files(directory, files, info, res):
    for name in ("sp_mann_pcoa_eig.tab", "sp_mann_pcoa_proj.tab"):
        path = os.path.join(directory, name)
        assert os.path.exists(path) == (name in files), name
        if name in files:
            assert open(path).read() == files[name], name
    for key, v in info.items():
        assert res[key] == v, key


def stage_case():
    names, table, order = cases.stage_samples()
    return names, table, order, pamcases.manhattan(table)


def test_stage_with_a_frequency_file_and_an_outlier(ctx, tmp_path):
    names, table, order, d = stage_case()
    dist_path, out, clus = clustered(ctx, tmp_path, names, d, freq=([names[i] for i in order], table[order].T))
    assert clus["status"] == CLUSTER_OK and clus["n_outliers"] == 1 and clus["n_samples"] == 40
    before = sorted(os.listdir(out))
    res = subpopr.pcoa_file(ctx, dist_path, out)
    files, info = model_files(names, d, out)
    check_files(out, files, info, res)
    assert res["status"] == PCOA_OK and res["n_samples"] == 44 and res["n_outliers"] == 1 and res["ms_kernel"] > 0
    assert sorted(os.listdir(out)) == sorted(before + list(files))    # nothing else written
    rows = [r.split("\t") for r in files["sp_mann_pcoa_proj.tab"].splitlines()]
    assert rows[0] == ["Axis.1", "Axis.2", "propFreqHomog", "clust"] and len(rows) == 45
    assert [r[0] for r in rows[1:]] == names[:44]                  # the outlier is in no row
    assert [r[4] for r in rows[41:]] == ["NA"] * 4 and set(r[4] for r in rows[1:41]) == {"1", "2"}      # the mixed samples were not clustered
    assert all(r[3] != "NA" and float(r[3]) < 0.8 for r in rows[41:]) and all(float(r[3]) >= 0.8 for r in rows[1:41])


def test_stage_without_a_frequency_file(ctx, tmp_path):
    names, table, order, d = stage_case()
    dist_path, out, clus = clustered(ctx, tmp_path, names, d)
    assert clus["status"] == CLUSTER_OK and clus["n_outliers"] == 1 and clus["n_samples"] == 44
    res = subpopr.pcoa_file(ctx, dist_path, out, species="sp")
    files, info = model_files(names, d, out)
    check_files(out, files, info, res)
    rows = [r.split("\t") for r in files["sp_mann_pcoa_proj.tab"].splitlines()[1:]]
    assert len(rows) == 44 and all(r[3] == "NA" for r in rows)


def test_stage_in_a_no_clustering_directory(ctx, tmp_path):
    names = pamcases.sample_names(40)
    d = pamcases.planted_dist(40, 0, 4)
    dist_path, out, clus = clustered(ctx, tmp_path, names, d, seed=7)
    assert clus["status"] == CLUSTER_NONE
    directory = os.path.join(out, "noClustering")
    res = subpopr.pcoa_file(ctx, dist_path, directory)
    files, info = model_files(names, d, directory)
    check_files(directory, files, info, res)
    rows = [r.split("\t") for r in files["sp_mann_pcoa_proj.tab"].splitlines()[1:]]
    assert len(rows) == 40 - clus["n_outliers"] and all(r[4] == "1" for r in rows)


def test_stage_on_collinear_samples_writes_no_projection(ctx, tmp_path):
    names = pamcases.sample_names(7)
    d = cases.line_dist(7)
    dist_path = str(tmp_path / "sp.filtered.mann.dist")
    pamcases.write_dist(dist_path, names, d)
    out = str(tmp_path / "out")
    os.makedirs(out)
    with open(os.path.join(out, "sp_mann_clustering.tab"), "w") as f:
        f.write(pammodel.clustering_text(names, [1] * 7))
    res = subpopr.pcoa_file(ctx, dist_path, out)
    files, info = model_files(names, d, out)
    assert sorted(files) == ["sp_mann_pcoa_eig.tab"] and info["status"] == model.TOO_FEW_AXES
    check_files(out, files, info, res)
    assert res["status"] == PCOA_TOO_FEW_AXES and res["k"] == 1
    assert files["sp_mann_pcoa_eig.tab"].splitlines()[1].split("\t")[2:] == ["1", "100"]


def test_the_launcher_writes_the_same_files(ctx, tmp_path):
    names, table, order, d = stage_case()
    dist_path, out, _ = clustered(ctx, tmp_path, names, d, freq=([names[i] for i in order], table[order].T))
    files, _ = model_files(names, d, out)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pcoaSubpops.py"), dist_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Species sp: 44 samples ordinated" in r.stdout
    for name, text in files.items():
        assert open(os.path.join(out, name)).read() == text, name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pcoaSubpops.py"), dist_path, str(tmp_path / "nowhere")], capture_output=True, text=True)
    assert r.returncode == 1 and "missing input file" in r.stderr
