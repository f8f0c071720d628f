"""Inputs shared by tests/test_pam_model.py and tests/test_gpu_cluster.py: planted-cluster SNV frequency tables, their Manhattan distance
matrices (exactly symmetric, zero diagonal), small-integer matrices with duplicated samples, the two input files of the stage, the large PAM
tasks (1755, 1756 and 4096 members) with the model's results for them, and freq tables whose cells sit on the band edges."""
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


def planted_dist_blocks(n, groups, seed, n_pos=12, noise=30.0):
    """manhattan(planted_freqs(...)) filled 256 rows at a time: the [n x n x n_pos] array of manhattan() would take 8 GB at n = 4096 and
    n_pos = 60.  Cell (i, j) is the same expression in the same order as cell (j, i), so the matrix is exactly symmetric, the diagonal 0."""
    p = planted_freqs(n, groups, seed, n_pos=n_pos, noise=noise)
    d = np.empty((n, n))
    for r in range(0, n, 256):
        d[r:r + 256] = np.abs(p[r:r + 256, None, :] - p[None, :, :]).mean(axis=2)
    return d


BAND_CELLS = (0.0, 4.999, 5.0, 10.0, 20.0, 50.0, 80.0, 90.0, 95.0, 95.001, 100.0, np.nan)
BAND_EDGES = (5.0, 10.0, 20.0, 80.0, 90.0, 95.0)                # computeSnvFreqStats is strict on both sides of each


def band_table(n_pos, s, seed):
    """A freq table [n_pos x s] for msnv_freq_bands_k: every cell one of BAND_CELLS (the six edges, a value just outside the outermost two,
    values inside and outside every band, NaN), and one column without a valid cell (its proportions are 0 / 0): the first column of the
    second block of 256 when there is one, the middle column otherwise."""
    rng = np.random.default_rng(seed)
    table = np.array(BAND_CELLS)[rng.integers(0, len(BAND_CELLS), size=(n_pos, s))]
    table[:, band_nan_column(s)] = np.nan
    return table


def band_nan_column(s):
    return 256 if s > 256 else s // 2


def integer_dist(n, seed, distinct=None, dim=3, top=3):
    """Small-integer distances with duplicated samples: ties and zero distances everywhere."""
    rng = np.random.default_rng(seed)
    distinct = distinct or max(2, n // 3)
    pts = rng.integers(0, top + 1, size=(distinct, dim))
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    p = pts[rng.permutation(pick)]
    return np.abs(p[:, None, :] - p[None, :, :]).sum(axis=2).astype(np.float64)


# ---- PAM tasks of 1755 / 1756 members (28 bytes of LDS per member: 49 140 and 49 168 bytes, on either side of 48 KiB) and of 4096, the cap.
# The matrices and the model's results are computed once per process and shared by test_pam_model.py, test_gpu_cluster.py and
# test_gpu_membstab.py; nobody writes to them.
LARGE_PAM = [(kind, m, k) for kind in ("real1756", "integer1756") for m in (1755, 1756) for k in (1, 2, 5)] + [("real4096", 4096, 1), ("real4096", 4096, 3)]
_large = {}


def large_matrix(kind):
    if kind not in _large:
        d = {"real1756": lambda: planted_dist_blocks(1756, 4, 21), "integer1756": lambda: integer_dist(1756, 22),
             "real4096": lambda: planted_dist_blocks(4096, 4, 21)}[kind]()
        d.setflags(write=False)
        _large[kind] = d
    return _large[kind]


def large_members(kind, m):
    """The task's index list: m of the matrix's samples in a shuffled order."""
    n = large_matrix(kind).shape[0]
    return np.random.default_rng(1000 + m).permutation(n)[:m].astype(np.int32)


def large_want(kind, m, k):
    """pammodel.pam of the task (large_members(kind, m), k): (medoids, cluster, n_swaps)."""
    import pammodel
    key = (kind, m, k)
    if key not in _large:
        ix = large_members(kind, m)
        _large[key] = pammodel.pam(large_matrix(kind)[np.ix_(ix, ix)], k)
    return _large[key]


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
