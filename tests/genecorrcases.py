"""Inputs shared by tests/test_genecorr_model.py (CPU, against scipy) and tests/test_gpu_genecorr.py (device against the model)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subpopr", "genecorr")
ABUND = os.path.join(GOLD, "refGenome3clus_allClust_relativeAbund.tab")
FIXTURE = {"pearson": os.path.join(GOLD, "refGenome3clus_corrGenes-pearson.tsv"), "spearman": os.path.join(GOLD, "refGenome3clus_corrGenes-spearman.tsv")}

# Worst distance of a numpy / scipy evaluation of each formula from the reference's own output over the fixtures' 400 rows
# per method (nObs = 150), times 10: R's pt, scipy's and the code under test are three evaluations of one function, and the
# margin leaves room for the third without letting a wrong formula through.  "rel": relative, "abs": absolute.
MARGIN = 10.0
BOUNDS = {
    ("pearson", "statistic"): ("rel", 3.9e-16 * MARGIN),
    ("pearson", "p.value"): ("rel", 1.14e-13 * MARGIN),
    ("pearson", "conf.int.low"): ("abs", 2.2e-16 * MARGIN),
    ("pearson", "conf.int.high"): ("abs", 2.2e-16 * MARGIN),
    ("pearson", "q.valueBH"): ("rel", 1.14e-13 * MARGIN),        # q comes from the code's own p and inherits p's relative distance (it is that
    ("spearman", "statistic"): ("rel", 0.0),                      # exact
    ("spearman", "p.value"): ("rel", 5.8e-14 * MARGIN),
    ("spearman", "q.valueBH"): ("rel", 5.8e-14 * MARGIN),        # p times N / rank, a factor exact to an ulp); BH itself is held to BH_BOUND
}
BH_BOUND = 2.5e-16 * MARGIN                                      # p.adjust(p, "BH") of the SAME p column: relative distance of q
RESULT_KEY = {"statistic": "statistic", "p.value": "p_value", "conf.int.low": "conf_low", "conf.int.high": "conf_high", "q.valueBH": "q_value"}


def read_fixture(method):
    lines = open(FIXTURE[method]).read().split("\n")
    header = lines[0].split("\t")
    rows = [ln.split("\t") for ln in lines[1:] if ln]
    cols = {h: [r[i] for r in rows] for i, h in enumerate(header)}
    return header, cols


def distance(kind, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = np.abs(got - want)
    if kind == "rel":
        d = np.where(want != 0, d / np.where(want != 0, np.abs(want), 1.0), d)
    return float(d.max())


def check_against_fixture(method, result, report=print):
    """result: corr_stats' dict for the fixture's estimates.  Prints every column's worst distance, then asserts its bound."""
    _, cols = read_fixture(method)
    worst = {}
    for (m, col), (kind, bound) in BOUNDS.items():
        if m == method:
            worst[col] = distance(kind, result[RESULT_KEY[col]], [float(x) for x in cols[col]])
            report("%s %s: worst %s distance from the fixture %.3g (bound %.3g)" % (method, col, kind, worst[col], bound))
    for (m, col), (kind, bound) in BOUNDS.items():
        if m == method:
            assert worst[col] <= bound, (method, col, worst[col], bound)
    return worst


SAMPLE_SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
N_GENES = 9
INVALID_GENE = 3


def make_case(n_samples, n_clusters, seed):
    """clust [K + 1 x S] (the last row the column sums) and 9 gene rows:
      0 all distinct   1 all zero but one cell   2 one long zero run, a few ties among the positives (the realistic shape)
      3 all cells equal and non-zero (invalid)   4 exactly two distinct values   5 equal to cluster 0 (rho = r = 1)
      6 cluster 0 mirrored, max + min - v (rho = -1)   7 small integers, many ties   8 sparse, all positives distinct
    With K = 3, cluster 2 is constant over the samples: all its rows are invalid.
    The positive values are lognormal over several decades, so a row's spread in log10 is far above 1e-3 of its magnitude:
    that keeps the two-pass centred sums well conditioned, which the 1e-11 bound on rho and r assumes."""
    rnd = np.random.RandomState(seed)
    s = n_samples
    clust = np.zeros((n_clusters + 1, s))
    for k in range(n_clusters):
        v = np.exp(rnd.normal(-2.0, 1.5, s))
        v[rnd.rand(s) < 0.3] = 0.0
        v[rnd.randint(s)] = 0.0
        v[(rnd.randint(s) + 1) % s] = 0.37                        # never constant
        clust[k] = v
    clust[0, :3] = (0.0, 0.21, 0.4)                               # three distinct cells also at S = 3
    if n_clusters == 3:
        clust[2] = 0.25
    clust[-1] = clust[:-1].sum(axis=0)
    genes = np.zeros((N_GENES, s))
    genes[0] = np.exp(rnd.normal(0.0, 2.0, s))
    genes[1, rnd.randint(s)] = 3.5
    n_pos = max(1, s - int(0.7 * s))
    pos = np.exp(rnd.normal(1.0, 2.0, n_pos))
    pos[: n_pos // 3] = pos[n_pos // 3: 2 * (n_pos // 3)][: n_pos // 3]      # ties among the positives
    genes[2, rnd.permutation(s)[:n_pos]] = pos
    genes[3] = 0.125
    genes[4] = np.where(rnd.rand(s) < 0.5, 0.002, 7.0)
    genes[4, 0], genes[4, 1] = 0.002, 7.0
    genes[5] = clust[0]
    genes[6] = clust[0].max() + clust[0].min() - clust[0]
    genes[7] = rnd.randint(0, 4, s).astype(np.float64)
    genes[7, :2] = (0.0, 3.0)
    genes[8, rnd.permutation(s)[:max(2, s // 5)]] = np.exp(rnd.normal(-3.0, 2.5, max(2, s // 5)))
    return clust, genes
