"""Inputs shared by tests/test_pam_model.py and tests/test_gpu_cluster.py: planted-cluster SNV frequency tables, their Manhattan distance
matrices (exactly symmetric, zero diagonal), small-integer matrices with duplicated samples, and the two input files of the stage."""
import numpy as np


def manhattan(points):
    """metaSNV's mann distance of complete rows: the mean absolute difference, the same sum order for (i, j) and (j, i)."""
    p = np.asarray(points, dtype=np.float64)
    return np.abs(p[:, None, :] - p[None, :, :]).mean(axis=2)


def planted_freqs(n, groups, seed, n_pos=60, noise=4.0):
    """n samples dealt round-robin into `groups` groups: every group has its own 0 / 100 allele pattern, every sample its own noise.
    Returns [n x n_pos] frequencies in [0, 100]."""
    rng = np.random.default_rng(seed)
    if groups:
        centers = rng.integers(0, 2, size=(groups, n_pos)) * 100.0
        base = centers[np.arange(n) % groups]
        u = rng.uniform(0, noise, size=(n, n_pos))
        return np.where(base > 50, base - u, base + u).round(3)
    return rng.uniform(0, 100, size=(n, n_pos)).round(3)


def planted_dist(n, groups, seed, **kw):
    return manhattan(planted_freqs(n, groups, seed, **kw))


def integer_dist(n, seed, distinct=None, dim=3, top=3):
    """Small-integer distances with duplicated samples: ties and zero distances everywhere."""
    rng = np.random.default_rng(seed)
    distinct = distinct or max(2, n // 3)
    pts = rng.integers(0, top + 1, size=(distinct, dim))
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    p = pts[rng.permutation(pick)]
    return np.abs(p[:, None, :] - p[None, :, :]).sum(axis=2).astype(np.float64)


def sample_names(n):
    return ["s%04d.bam" % (i + 1) for i in range(n)]


def write_dist(path, names, d):
    """<species>.filtered.mann.dist as metaSNV_DistDiv.py --dist writes it (DataFrame.to_csv(sep='\\t'))."""
    with open(path, "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        for i, nm in enumerate(names):
            f.write(nm + "\t" + "\t".join(repr(float(v)) for v in d[i]) + "\n")


def write_freq(path, names, table):
    """<species>.filtered.freq: positions x samples, -1 where a sample has no coverage (NaN here)."""
    with open(path, "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        for p, row in enumerate(table):
            f.write("c1:-:%d:A:." % (p + 1) + "\t" + "\t".join("-1" if v != v else repr(float(v)) for v in row) + "\n")
