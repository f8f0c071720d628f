"""Inputs of tests/test_gpu_subpopr_run.py: a table for the cluster stage's -x / -y with cells on the edges of the 10/90 and 20/80 bands, and metaSNV
projects of a few small species (the shape of test_gpu_profile.py's chain: 0/1 planted frequencies plus a few uninformative rows, called_SNPs written to
match)."""
import os

import numpy as np

import genotypecases
import pamcases
import profilecases

N = 24                                                         # samples per species
# 24 samples cannot reach the default prediction-strength cut: predStrengthCustom leaves a half's last entry out of the numerator, so the cluster of m
# members that holds it scores (m - 2) / m, 0.667 for the 6 a half of 12 gives a subspecies.  The planted species score 0.667 at k = 2, the ones
# without structure 0.32 to 0.36 (tests/pammodel.py), so the runs here cut at 0.5.
PS_CUT = 0.5
DRIVER_OPTS = ["--stability-iters", "2", "--boot", "5", "--minNumSamples", "12", "--seed", "7", "--clusterPSThreshold", "0.5"]
STAGE_OPTS = dict(seed=7, stability_iters=2, ps_cut=PS_CUT)


# ---------------------------------------------------------------------------------------------- the cluster stage's filter
# (cells on 10 / 90, cells on 20 / 80, cells without coverage) of the samples that are not plain; 40 positions
EDGE_SAMPLES = {2: (8, 0, 0),       # 32 / 40 = 0.8 outside 10/90: kept at -x 0.1 (>=), 40 / 40 at -x 0.2
                5: (9, 0, 0),       # 31 / 40 at -x 0.1: dropped; 40 / 40 at -x 0.2: kept
                7: (0, 8, 0),       # 32 / 40 at both: kept
                11: (0, 9, 0),      # 31 / 40 at both: dropped
                13: (5, 4, 0),      # 31 / 40 at -x 0.1: dropped; 36 / 40 at -x 0.2: kept
                17: (0, 6, 10),     # 24 / 30 = 0.8 of the covered cells at both: kept
                19: (0, 0, 40)}     # no covered cell: 0 / 0, never kept


def band_edge_table():
    """(names, distances [24 x 24], freq-table sample order, table [40 x 24] on the percent scale with NaN for no coverage).  Two planted groups with
    cells in 0..4 and 96..100; the samples of EDGE_SAMPLES have some cells moved onto the bands' edges (low cells to 10 or 20, high ones to 90 or 80)."""
    rng = np.random.default_rng(31)
    n_pos = 40
    names = pamcases.sample_names(N)
    centers = rng.integers(0, 2, size=(2, n_pos))
    high = centers[np.arange(N) % 2].T.astype(bool)             # [n_pos x N]
    jitter = rng.integers(0, 5, size=(n_pos, N)).astype(np.float64)
    table = np.where(high, 100.0 - jitter, jitter)
    dist = pamcases.manhattan(table.T)
    for s, (n10, n20, n_nan) in EDGE_SAMPLES.items():
        rows = rng.permutation(n_pos)
        for p in rows[:n10]:
            table[p, s] = 90.0 if high[p, s] else 10.0
        for p in rows[n10:n10 + n20]:
            table[p, s] = 80.0 if high[p, s] else 20.0
        for p in rows[n10 + n20:n10 + n20 + n_nan]:
            table[p, s] = np.nan
    order = [int(i) for i in np.random.default_rng(32).permutation(N)]
    return names, dist, order, table


def strict_proportion(column, x):
    """computeSnvFreqStatsThreshold of one sample column on the percent scale, in double as R computes it."""
    h = 1.0 - x if x > 0.5 else x
    t = h * 100.0
    hi, lo = max(100.0 - t, t), min(100.0 - t, t)
    covered = column[~np.isnan(column)]
    with np.errstate(invalid="ignore"):
        return np.float64(np.count_nonzero((covered < lo) | (covered > hi))) / np.float64(covered.size)


# ---------------------------------------------------------------------------------------------- projects
def planted_species(seed, n=N, groups=2, n_pos=16, n_noise=6):
    """A frequency table [n_pos + n_noise x n] on metaSNV's [0, 1] scale: groups > 0: position p carries its alternative allele in group p % groups
    alone, then n_noise rows that tell nothing; groups = 0: no structure at all."""
    rng = np.random.default_rng(seed)
    if groups:
        truth = np.arange(n) % groups
        table = np.where(truth[None, :] == (np.arange(n_pos) % groups)[:, None], 1.0, 0.0)
        return np.concatenate([table, rng.uniform(0.3, 0.7, size=(n_noise, n)).round(3)])
    return rng.uniform(0.0, 1.0, size=(n_pos + n_noise, n)).round(3)


def called_snps_text(contig, table, seed):
    """called_SNPs lines that give back `table` (positions x all samples) at depths of 20 to 39."""
    rng = np.random.default_rng(seed)
    out = []
    for p, row in enumerate(table):
        cov = rng.integers(20, 40, size=len(row))
        alt = np.rint(cov * row).astype(int)
        out.append("%s\t-\t%d\tT\t%s\t%d|A|.|%s\n" % (contig, 10 * p + 7, "|".join(map(str, cov)), alt.sum(), "|".join(map(str, alt))))
    return "".join(out)


def labels_of(contig, n_rows):
    return ["%s:-:%d:T>A:." % (contig, 10 * p + 7) for p in range(n_rows)]


def write_species(proj, sp, names, table, dist_names=None, dist=None, freq_columns=None):
    """<proj>/distances/<sp>.filtered.mann.dist (text cells may be given) and <proj>/filtered/pop/<sp>.filtered.freq of the columns freq_columns."""
    os.makedirs(os.path.join(proj, "distances"), exist_ok=True)
    os.makedirs(os.path.join(proj, "filtered", "pop"), exist_ok=True)
    if dist is None:
        dist_names, dist = names, [[repr(float(v)) for v in row] for row in pamcases.manhattan(table.T)]
    with open(os.path.join(proj, "distances", sp + ".filtered.mann.dist"), "w") as f:
        f.write("\t" + "\t".join(dist_names) + "\n")
        for nm, row in zip(dist_names, dist):
            f.write(nm + "\t" + "\t".join(row) + "\n")
    cols = list(range(len(names))) if freq_columns is None else freq_columns
    genotypecases.write_freq(os.path.join(proj, "filtered", "pop", sp + ".filtered.freq"), [names[c] for c in cols], labels_of("ctg" + sp, len(table)), table[:, cols])


EXTRA, MISSING = "zz_extra.bam", 3                             # species 404: a sample with blank distance cells, and the column its frequency table lacks


def five_species_project(proj, by_hand=False):
    """101: two planted subspecies; 202: no structure; 303: 8 samples; 404: 101's tables with one more sample whose distance cells are blank and one
    sample missing from the frequency table (by_hand: the two removed from the distance table instead); 505: a distance file only.  Returns the paths
    of the species-abundance and gene-family tables."""
    names = genotypecases.sample_names(N)
    os.makedirs(os.path.join(proj, "snpCaller"))
    open(os.path.join(proj, "all_samples"), "w").write(profilecases.all_samples_text(names))
    t101, t202, t303 = planted_species(5), planted_species(6, groups=0), planted_species(8)
    snps = ""
    if not by_hand:
        write_species(proj, "101", names, t101)
        write_species(proj, "202", names, t202)
        write_species(proj, "303", names, t303, freq_columns=list(range(8)), dist_names=names[:8],
                      dist=[[repr(float(v)) for v in row] for row in pamcases.manhattan(t303[:, :8].T)])
        open(os.path.join(proj, "distances", "505.filtered.mann.dist"), "w").write("\t" + "\t".join(names[:2]) + "\n" + names[0] + "\t0.0\t0.5\n" + names[1] + "\t0.5\t0.0\n")
        snps += called_snps_text("ctg101", t101, 101) + called_snps_text("ctg202", t202, 202) + called_snps_text("ctg303", t303, 303)
    d = [[repr(float(v)) for v in row] for row in pamcases.manhattan(t101.T)]
    keep = [c for c in range(N) if c != MISSING]
    if by_hand:
        write_species(proj, "404", names, t101, dist_names=[names[c] for c in keep], dist=[[d[i][j] for j in keep] for i in keep], freq_columns=keep)
    else:
        blank = [row + [""] for row in d] + [[""] * N + ["0.0"]]
        write_species(proj, "404", names, t101, dist_names=names + [EXTRA], dist=blank, freq_columns=keep)
    snps += called_snps_text("ctg404", t101, 404)
    open(os.path.join(proj, "snpCaller", "called_SNPs.best_split_1"), "w").write(snps)
    rng = np.random.default_rng(9)
    abund_path, gene_path = os.path.join(proj, "species.tsv"), os.path.join(proj, "genes.tsv")
    abund = rng.uniform(0.01, 0.2, size=(4, N)).round(4)
    open(abund_path, "w").write("\t" + "\t".join(names) + "\n" + "".join(
        sp + "\t" + "\t".join(repr(float(v)) for v in row) + "\n" for sp, row in zip(("101", "202", "303", "404"), abund)))
    genes = rng.uniform(1, 50, size=(5, N)).round(3)
    genes[0] = np.where(np.arange(N) % 2 == 0, abund[0] * 1000, 0.001).round(6)          # a gene family that follows 101's first subspecies
    open(gene_path, "w").write("gene\t" + "\t".join(names) + "\n" + "".join("g%d\t%s\n" % (i, "\t".join(repr(float(v)) for v in row)) for i, row in enumerate(genes)))
    return abund_path, gene_path


def two_species_project(proj):
    """101 as above and 909, whose frequency table holds a cell above 1 (an old metaSNV's percent scale)."""
    names = genotypecases.sample_names(N)
    os.makedirs(os.path.join(proj, "snpCaller"))
    open(os.path.join(proj, "all_samples"), "w").write(profilecases.all_samples_text(names))
    t101, t909 = planted_species(5), planted_species(5)
    write_species(proj, "101", names, t101)
    t909[3, 4] = 100.0
    write_species(proj, "909", names, t909)
    open(os.path.join(proj, "snpCaller", "called_SNPs.best_split_1"), "w").write(called_snps_text("ctg101", t101, 101))


def read_tree(root, skip=()):
    out = {}
    for dp, _, files in os.walk(root):
        for f in files:
            rel = os.path.relpath(os.path.join(dp, f), root)
            if not any(rel.startswith(s) for s in skip):
                out[rel] = open(os.path.join(dp, f), "rb").read()
    return out
