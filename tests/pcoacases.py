"""Inputs shared by tests/test_pcoa_model.py and tests/test_gpu_pcoa.py: distance matrices whose ordination is known without a solver, the planted and
integer matrices of tests/pamcases.py at the sizes where the kernels' loops change shape, the model's results for them (computed once per process,
never written to), and the samples of the file stage."""
import numpy as np

import pamcases
import pcoamodel

KINDS = ("manhattan", "euclidean", "integer")
EIGH_SIZES = (3, 7, 8, 63, 64, 65, 129, 200)
# the device's sizes: one pair; the bye (3, 5); 4; 32 pairs and one more or fewer (63, 64, 65); a wavefront of pairs and one more (127 .. 130)
GPU_SIZES = (2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130)


def euclidean(points):
    """Exactly symmetric: (a - b)^2 == (b - a)^2, summed in the same order for (i, j) and (j, i)."""
    p = np.asarray(points, dtype=np.float64)
    diff = p[:, None, :] - p[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2))


def grid_dist():
    """The 3 x 4 unit grid: eigenvalues 15 (the axis of four) and 8 (the axis of three), the rest 0."""
    return euclidean([(x, y) for y in range(3) for x in range(4)])


def line_dist(n=7):
    """n points at 0 .. n - 1 on a line: one eigenvalue, 28 for n = 7."""
    return euclidean([(x,) for x in range(n)])


def matrix(kind, n):
    if kind == "manhattan":
        return pamcases.planted_dist(n, 3, 100 + n, noise=30.0)
    if kind == "euclidean":
        return euclidean(pamcases.planted_freqs(n, 3, 100 + n, noise=30.0))
    return pamcases.integer_dist(n, 200 + n)


_want = {}


def solved(kind, n):
    """B, its trace and the Jacobi solve of it: (b, trace, diagonal, V, sweeps, rotations)."""
    if ("solved", kind, n) not in _want:
        b, trace = pcoamodel.centre(matrix(kind, n))
        _want[("solved", kind, n)] = (b, trace) + pcoamodel.jacobi(b)
    return _want[("solved", kind, n)]


def want(kind, n):
    """pcoamodel.pcoa(matrix(kind, n), n): every axis, so the first two columns are what n_axes = 2 gives."""
    if (kind, n) not in _want:
        res = pcoamodel.pcoa(matrix(kind, n), n, solved=solved(kind, n))
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[(kind, n)] = res
    return _want[(kind, n)]


def stage_samples():
    """45 samples in two planted groups: 40 clean ones, four with a third of their SNVs mixed (below 0.8 at 10 / 90: not clustered, NA in clust) and
    one unlike every other (the outlier: in no row).  Returns names, the table [samples x positions] and the order of the freq file's columns."""
    names = pamcases.sample_names(45)
    table = pamcases.planted_freqs(45, 2, 8)
    table[40:44, ::3] = 45.0
    table[44] = 100.0 - table[44]
    order = list(np.random.default_rng(1).permutation(45))
    return names, table, order
