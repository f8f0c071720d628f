"""bench.py --dump-outputs writer: the dense form of the weak line and the cell form of the strong line give the same arrays, in float32 /
float64, within the size limit (a fixed seeded sample of the sites beyond it)."""
import os

import numpy as np

import bench
from metasnv_amd import core


def _case(n=3000, ns=7, seed=1):
    rng = np.random.default_rng(seed)
    sites = np.zeros(n, core.SITE_DTYPE)
    sites["tid"], sites["pos"], sites["refchar"] = rng.integers(0, 3, n), np.arange(n), 65
    sites["n"] = rng.integers(0, 50, (n, 4))
    dense = np.zeros((n, ns), core.SAMPLE_DTYPE)
    mask = rng.random((n, ns)) < 0.3
    dense["cov"][mask] = rng.integers(1, 100, mask.sum())
    dense["n"][mask] = rng.integers(0, 9, (mask.sum(), 4))
    return sites, dense


def test_dense_and_cell_forms_dump_the_same_arrays(tmp_path, monkeypatch):
    sites, dense = _case()
    ns = dense.shape[1]
    row_off, cell_sample, cells = core.dense_to_cells(dense)
    last = dict(n_sites=len(sites), n_called_pop=5, n_called_indiv=6, n_events=7, n_overflow=0, algorithmic_bytes=123)
    for limit in (64 << 20, 200000):
        monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
        a, b = tmp_path / ("a%d" % limit), tmp_path / ("b%d" % limit)
        bench.dump_outputs(str(a), sites, lambda idx: dense[idx], ns, last)
        bench.dump_outputs(str(b), sites, bench.cell_rows(ns, row_off, cell_sample, cells), ns, last)
        names = sorted(os.listdir(a))
        assert names == ["pass_counts.npy", "site_index.npy", "site_samples.npy", "sites.npy"]
        assert sum(os.path.getsize(a / f) for f in names) <= limit
        for f in names:
            x, y = np.load(a / f), np.load(b / f)
            assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and (x == y).all(), f
        idx = np.load(a / "site_index.npy").astype(np.int64)
        assert (len(idx) == len(sites)) == (limit == 64 << 20) and (np.diff(idx) > 0).all()
        smp, cols = np.load(a / "site_samples.npy"), np.load(a / "sites.npy")
        assert (smp[..., 0] == dense["cov"][idx]).all() and (smp[..., 1:] == dense["n"][idx]).all()
        assert (cols[:, 1] == sites["pos"][idx]).all() and (cols[:, 3:7] == sites["n"][idx]).all()
        assert list(np.load(a / "pass_counts.npy")) == [float(last[k]) for k in bench.PASS_COUNTS]
