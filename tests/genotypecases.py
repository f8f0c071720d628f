"""Inputs shared by tests/test_genotype_model.py and tests/test_gpu_genotype.py: SNV frequency tables with planted genotyping positions and
the two input files of the stage.  (pamcases.planted_freqs does not serve: a random 0 / 100 pattern distinct from all others is rare, so it
yields no genotyping position for three clusters or more.)"""
import numpy as np


def planted_genotypes(n_samples, n_clusters, rows_per_cluster, background, seed, na_share=0.0):
    """Samples dealt round-robin into n_clusters clusters (clust[s] = s % n_clusters + 1).  Per cluster a block of rows_per_cluster rows where
    its samples sit near 100 and all others near 0 -- the other way round on every second row of the block: the flips -- then `background`
    rows of uniform noise; NaN scattered at na_share.  Returns (table [P x S] in [0, 100], 3 decimals; clust [S])."""
    rng = np.random.default_rng(seed)
    clust = np.arange(n_samples) % n_clusters + 1
    blocks = []
    for c in range(1, n_clusters + 1):
        u = rng.uniform(0, 4, size=(rows_per_cluster, n_samples))
        high = np.broadcast_to(clust == c, u.shape).copy()
        high[1::2] = ~high[1::2]
        blocks.append(np.where(high, 100.0 - u, u))
    blocks.append(rng.uniform(0, 100, size=(background, n_samples)))
    table = np.concatenate(blocks).round(3)
    table[rng.uniform(size=table.shape) < na_share] = np.nan
    return table, clust


def sample_names(n):
    return ["s%04d.bam" % (i + 1) for i in range(n)]


def row_labels(n):
    return ["c1:-:%d:A:." % (p + 1) for p in range(n)]


def write_freq(path, names, labels, table):
    """<species>.filtered.freq: positions x samples in 0..1, -1 where a sample has no coverage (NaN here)."""
    with open(path, "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        for lab, row in zip(labels, table):
            f.write(lab + "\t" + "\t".join("-1" if v != v else repr(float(v)) for v in row) + "\n")
