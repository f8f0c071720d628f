"""tests/pcoamodel.py, the rule the device is compared with bit for bit (tests/test_gpu_pcoa.py), against what is known without it: the schedule's
combinatorics, ordinations with closed-form eigenvalues, and numpy.linalg.eigh on the centred matrix.

The bounds of the eigh comparison: both solvers are backward stable, each eigenvalue within about n 2^-52 max |lambda| of the exact one, so the two
differ by at most the sum; 4 n 2^-52 max |lambda| leaves a factor of two.  The residual max |B V - V Lambda| and the orthogonality max |V^T V - I| of a
Jacobi solve grow with n 2^-52 as well (each cell takes n - 1 rotations per sweep, each with a relative error of a few 2^-53)."""
import itertools

import numpy as np
import pytest

import pcoacases as cases
import pcoamodel as model

EPS = 2.0 ** -52


@pytest.mark.parametrize("n", list(range(2, 11)) + [63, 64, 65])
def test_a_sweep_holds_every_pair_once_and_a_step_only_disjoint_pairs(n):
    m = n + (n & 1)
    seen = []
    for r in range(m - 1):
        pairs = model.step_pairs(n, r)
        assert len(pairs) == m // 2 and all(p < q for p, q in pairs)
        full = [(p, q) for p, q in pairs if q < n]
        assert len(full) == n // 2 and all(q < n for p, q in pairs[1:])                  # only slot 0 can be the bye
        touched = [i for pq in full for i in pq] + [p for p, q in pairs if q >= n]
        assert sorted(touched) == list(range(n))                   # disjoint, and nobody sits a step out but the bye
        seen += full
    assert sorted(seen) == list(itertools.combinations(range(n), 2))


def close(got, want, lam1):
    return np.abs(np.asarray(got) - np.asarray(want)).max() <= 64 * EPS * lam1


def test_the_unit_grid_has_eigenvalues_15_and_8_and_its_axes_give_the_distances_back():
    d = cases.grid_dist()
    res = model.pcoa(d, 2)
    assert res["status"] == model.OK and res["k"] == 2 and res["n_negative"] == 0
    assert close(res["eig"], [15.0, 8.0] + [0.0] * 10, 15.0)
    assert res["eig"][2:].tolist() == [0.0] * 10                   # the cut-off made them exact zeros
    assert close(res["rel_eig"][:2], [15.0 / 23.0, 8.0 / 23.0], 1.0) and close(res["axis_pct"][:2], [1500.0 / 23.0, 800.0 / 23.0], 100.0)
    back = cases.euclidean(res["vectors"])
    print("grid: max |D' - D| = %.3g" % np.abs(back - d).max())
    assert close(back, d, 15.0)
    for a in range(2):                                             # the sign rule
        col = res["vectors"][:, a]
        assert col[np.argmax(np.abs(col))] > 0


def test_points_on_a_line_have_one_axis():
    res = model.pcoa(cases.line_dist(7), 2)
    assert close(res["eig"], [28.0] + [0.0] * 6, 28.0) and res["eig"][1:].tolist() == [0.0] * 6
    assert res["status"] == model.TOO_FEW_AXES and res["k"] == 1
    assert np.isnan(res["vectors"][:, 1]).all() and close(np.abs(res["vectors"][:, 0]), np.abs(np.arange(7) - 3.0), 28.0)


def test_two_samples():
    res = model.pcoa(np.array([[0.0, 3.0], [3.0, 0.0]]), 2)
    assert close(res["eig"], [4.5, 0.0], 4.5) and res["eig"][1] == 0.0 and res["k"] == 1 and res["status"] == model.TOO_FEW_AXES


def test_the_zero_matrix_is_exact():
    res = model.pcoa(np.zeros((5, 5)), 2)
    assert res["eig"].tolist() == [0.0] * 5 and res["rotations"] == 0 and res["sweeps"] == 1
    assert res["status"] == model.TOO_FEW_AXES and res["k"] == 0 and np.isnan(res["vectors"]).all()
    assert np.isnan(res["rel_eig"]).all() and np.isnan(res["axis_pct"]).all()      # 0 / 0, as R has it


def test_the_files_of_the_stage():
    import pamcases
    import pammodel
    names = pamcases.sample_names(12)
    clustering = pammodel.clustering_text(names[:10], [1, 2] * 5)
    composition = "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95\n" + "".join("%s\t1\t%s\t0.5\n" % (nm, "NaN" if i == 3 else "0.875")
                                                                                                  for i, nm in enumerate(names[:11]))
    files, info = model.pcoa_files(names, cases.grid_dist(), "sp", clustering, composition)
    assert info == {"status": model.OK, "sweeps": info["sweeps"], "rotations": info["rotations"], "k": 2, "n_negative": 0, "n_samples": 12, "n_outliers": 0}
    eig = files["sp_mann_pcoa_eig.tab"].splitlines()
    assert eig[0] == "Eigenvalues\tRelative_eig\taxisPercent" and len(eig) == 13
    assert eig[1] == "1\t15\t0.652173913043478\t65.2173913043478" and eig[2] == "2\t8\t0.347826086956522\t34.7826086956522" and eig[12] == "12\t0\t0\t0"
    proj = [r.split("\t") for r in files["sp_mann_pcoa_proj.tab"].splitlines()]
    assert proj[0] == ["Axis.1", "Axis.2", "propFreqHomog", "clust"] and [r[0] for r in proj[1:]] == names
    assert [r[3] for r in proj[1:]] == ["0.875"] * 3 + ["NaN"] + ["0.875"] * 7 + ["NA"]           # a sample the composition file does not list
    assert [r[4] for r in proj[1:]] == ["1", "2"] * 5 + ["NA", "NA"]                               # samples the clustering does not list
    files, info = model.pcoa_files(names[:7], cases.line_dist(7), "sp", clustering)
    assert sorted(files) == ["sp_mann_pcoa_eig.tab"] and info["status"] == model.TOO_FEW_AXES    # "Error during pcoa": no projection


@pytest.mark.skipif(__import__("metasnv_amd.core", fromlist=["core"]).device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_launcher_refuses_to_run_without_a_gpu(tmp_path):
    import os
    import subprocess
    import sys
    import pamcases
    import pammodel
    names = pamcases.sample_names(7)
    dist = tmp_path / "sp.filtered.mann.dist"
    pamcases.write_dist(str(dist), names, cases.line_dist(7))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "pcoaSubpops.py"), str(dist), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "missing input file" in r.stderr            # no clustering yet
    (tmp_path / "sp_mann_clustering.tab").write_text(pammodel.clustering_text(names, [1] * 7))
    r = subprocess.run([sys.executable, os.path.join(root, "pcoaSubpops.py"), str(dist), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["sp.filtered.mann.dist", "sp_mann_clustering.tab"]


@pytest.mark.parametrize("n", cases.EIGH_SIZES)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_against_eigh(kind, n):
    d = cases.matrix(kind, n)
    b, trace, lam, v, sweeps, rotations = cases.solved(kind, n)
    assert (b == b.T).all()
    want = np.linalg.eigh(b)[0]
    top = np.abs(want).max()
    err_eig = np.abs(np.sort(lam) - want).max() / (EPS * top)
    err_res = np.abs(b @ v - v * lam[None, :]).max() / (EPS * top)
    err_orth = np.abs(v.T @ v - np.eye(n)).max() / EPS
    print("%s n=%d: %d sweeps, %d rotations; eigenvalues %.2f, residual %.2f (x 2^-52 max |lambda|), orthogonality %.2f n 2^-52"
          % (kind, n, sweeps, rotations, err_eig, err_res, err_orth / n))
    assert err_eig <= 4 * n and err_res <= 4 * n and err_orth <= 4 * n and sweeps <= 64
    res = cases.want(kind, n)
    assert (np.diff(res["eig"]) <= 0).all() and res["sweeps"] == sweeps and res["rotations"] == rotations
    if kind == "manhattan" and n > 3:
        # the branch real data takes: a Manhattan distance is no Euclidean one.  Not at n = 3: three points of any metric embed in a plane, so
        # their centred matrix has no negative eigenvalue
        assert res["n_negative"] > 0 and want.min() < -model.CUT
    if kind == "integer":
        assert (d == 0).sum() > n                                  # duplicated samples
