"""numpy-only restatement of subpopr's correlateSubpopProfileWithGeneProfiles
(src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R): what msnv_gene_corr, msnv_corr_stats and msnv_gene_corr_files compute.

Average ranks, both coefficients, cor.test's derived columns, p.adjust(method="BH"), selectSubspeciesSpecificGenes and the
text writer.  The t tail is a continued fraction (modified Lentz) behind a gamma-function ratio: GPU tests import this module, so it
must not need scipy."""
import math

import numpy as np

QNORM_975 = 1.959963984540054
PEARSON_HEADER = "geneFamily\tcluster\tstatistic\tp.value\testimate\tnull.value\talternative\tmethod\tconf.int\tconf.int.low\tconf.int.high\tnObs\tq.valueBH"
SPEARMAN_HEADER = "geneFamily\tcluster\tstatistic\tp.value\testimate\tnull.value\talternative\tmethod\tnObs\tq.valueBH"
GROUP_HEADER = "geneFamily\tcluster\tgeneIsCorrelated\tgeneIsNotCorrelated"


# ------------------------------------------------------------------------------------------------ coefficients
def average_ranks(v):
    """rank(v, ties.method = "average")"""
    v = np.asarray(v, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    sv = v[order]
    n = len(v)
    start = np.r_[True, sv[1:] != sv[:-1]]
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    end = np.r_[sv[1:] != sv[:-1], True]
    last = np.minimum.accumulate(np.where(end, np.arange(n), n - 1)[::-1])[::-1]
    ranks = np.empty(n)
    ranks[order] = (first + last + 2) / 2.0
    return ranks


def _coef(dx, dy):
    c = float(np.sum(dx * dy) / math.sqrt(float(np.sum(dx * dx)) * float(np.sum(dy * dy))))
    return max(-1.0, min(1.0, c))


def pseudocount_of(genes):
    genes = np.asarray(genes, dtype=np.float64)
    return float(genes[genes > 0].min()) / 1000.0


def gene_correlations(clust, genes):
    """clust [K1 x S], genes [G x S] -> rho, r, valid [K1 x G] and the pseudocount (doCorr, :141-153)."""
    clust = np.asarray(clust, dtype=np.float64)
    genes = np.asarray(genes, dtype=np.float64)
    k1, s = clust.shape
    g = genes.shape[0]
    pc = pseudocount_of(genes)
    mr = (s + 1) / 2.0

    def prep(row):
        lg = np.log10(row + pc)
        return average_ranks(row) - mr, lg - lg.sum() / s, row.max() != row.min()
    cl = [prep(row) for row in clust]
    rho, r = np.full((k1, g), np.nan), np.full((k1, g), np.nan)
    valid = np.zeros((k1, g), dtype=bool)
    for j in range(g):
        dr, dl, ok = prep(genes[j])
        for c in range(k1):
            if ok and cl[c][2]:
                valid[c, j] = True
                rho[c, j] = _coef(cl[c][0], dr)
                r[c, j] = _coef(cl[c][1], dl)
    return {"rho": rho, "r": r, "valid": valid, "pseudocount": pc}


# ------------------------------------------------------------------------------------------------ cor.test's derived columns
def _beta_cf(a, b, x):
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 20001):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = tiny if abs(d) < tiny else d
        c = 1.0 + aa / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = tiny if abs(d) < tiny else d
        c = 1.0 + aa / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 3e-16:
            break
    return h


def gamma_ratio(a):
    """Gamma(a + 1/2) / Gamma(a) to an ulp or two: shifted up to a >= 20 by the recurrence, then the asymptotic series.  The
    difference of two lgamma values of size 250 (df = 148) would leave 1e-13 of relative error in the density, and ten times that in a
    p of 0.09 taken as 1 - I."""
    pr, z = 1.0, float(a)
    while z < 20.0:
        pr *= z / (z + 0.5)
        z += 1.0
    w = 1.0 / z
    w2 = w * w
    return pr * math.sqrt(z) * math.exp(w * (-1.0 / 8.0 + w2 * (1.0 / 192.0 + w2 * (-1.0 / 640.0 + w2 * (17.0 / 14336.0 + w2 * (-31.0 / 18432.0))))))


def t_statistic(method, e, df):
    """cor.test's t: sqrt(df) r / sqrt(1 - r^2) for pearson, r / sqrt((1 - r^2) / df) for spearman -- each with R's own rounding"""
    u = 1.0 - e * e
    if u <= 0.0:
        return math.copysign(math.inf, e)
    if method == "pearson":
        return math.sqrt(df) * e / math.sqrt(u)
    return e / math.sqrt(u / df)


SQRT_PI = 1.7724538509055159


def t_two_sided(t, df):
    """min(1, 2 P(T_df >= |t|)) = I_x(df / 2, 1 / 2) at x = df / (df + t^2)"""
    if math.isinf(t):
        return 0.0
    if t == 0.0:
        return 1.0
    t2 = t * t
    x, y, a, b = df / (df + t2), t2 / (df + t2), 0.5 * df, 0.5
    lx = math.log1p(-y) if y < 0.5 else math.log(x)
    front = math.exp(a * lx) * math.sqrt(y) * gamma_ratio(a) / SQRT_PI      # x^a y^b / B(a, b)
    if x < (a + 1.0) / (a + b + 2.0):
        p = front * _beta_cf(a, b, x) / a
    else:
        p = 1.0 - front * _beta_cf(b, a, y) / b
    return min(1.0, max(0.0, p))


def bh(p):
    """p.adjust(p, "BH")"""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    if n == 0:
        return p.copy()
    o = np.argsort(-p, kind="stable")
    q = np.empty(n)
    q[o] = np.minimum(1.0, np.minimum.accumulate((n / np.arange(n, 0, -1.0)) * p[o]))
    return q


def corr_stats(method, estimate, n_obs):
    est = np.asarray(estimate, dtype=np.float64).ravel()
    nobs = np.broadcast_to(np.asarray(n_obs, dtype=np.int64), est.shape)
    stat, p = np.empty(len(est)), np.empty(len(est))
    lo, hi = np.full(len(est), np.nan), np.full(len(est), np.nan)
    for i, (e, n) in enumerate(zip(est.tolist(), nobs.tolist())):
        df = n - 2.0
        if method == "pearson":
            stat[i] = math.copysign(math.inf, e) if abs(e) >= 1.0 else t_statistic(method, e, df)
            if n > 3 and abs(e) < 1.0:
                z, s = math.atanh(e), QNORM_975 / math.sqrt(n - 3.0)
                lo[i], hi[i] = math.tanh(z - s), math.tanh(z + s)
            elif n > 3:
                lo[i] = hi[i] = math.copysign(1.0, e)
        else:
            stat[i] = (float(n) ** 3 - n) * (1.0 - e) / 6.0
        p[i] = 0.0 if abs(e) >= 1.0 else t_two_sided(t_statistic(method, e, df), df)
    out = {"statistic": stat, "p_value": p, "q_value": bh(p)}
    if method == "pearson":
        out["conf_low"], out["conf_high"] = lo, hi
    return out


# ------------------------------------------------------------------------------------------------ text
def r_number(v):
    """The shortest digits that read back to the same double, the exponent unpadded (1e-8, not 1e-08)."""
    v = float(v)
    if v != v:
        return "NA"
    if math.isinf(v):
        return "Inf" if v > 0 else "-Inf"
    t = repr(v)
    if "e" in t:
        m, e = t.split("e")
        sign = e[0] if e[0] in "+-" else ""
        t = m + "e" + sign + (e.lstrip("+-").lstrip("0") or "0")
    return t


def table_text(method, rows):
    """rows: dicts with gene, cluster, statistic, p, estimate, n_obs, q (and lo, hi for pearson)."""
    out = [PEARSON_HEADER if method == "pearson" else SPEARMAN_HEADER]
    for w in rows:
        f = [w["gene"], w["cluster"], r_number(w["statistic"]), r_number(w["p"]), r_number(w["estimate"]), "0", "two.sided", method]
        if method == "pearson":
            f += ["FALSE", r_number(w["lo"]), r_number(w["hi"])]
        f += [str(int(w["n_obs"])), r_number(w["q"])]
        out.append("\t".join(f))
    return "\n".join(out) + "\n"


def groups_text(rows):
    out = [GROUP_HEADER]
    for gene, cluster, corr, notc in rows:
        out.append("\t".join([gene, cluster, "TRUE" if corr else "FALSE", "TRUE" if notc else "FALSE"]))
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------------------------------------ the file form
class NoClusters(Exception):
    pass


def read_cluster_table(path):
    lines = [ln.rstrip("\r\n") for ln in open(path) if ln.strip("\r\n")]
    names = lines[0].split("\t")
    samples, vals = [], []
    for ln in lines[1:]:
        f = ln.split("\t")
        assert len(f) == len(names) + 1
        samples.append(f[0])
        vals.append([float(x) for x in f[1:]])
    return names, samples, np.array(vals, dtype=np.float64).reshape(len(samples), len(names))


def read_gene_table(path):
    lines = [ln.rstrip("\r\n") for ln in open(path) if ln.strip("\r\n") and not ln.startswith("#")]
    cols = [c.strip(" ") for c in lines[0].split("\t")[1:]]
    ids, vals = [], []
    for ln in lines[1:]:
        f = ln.split("\t")
        ids.append(f[0].strip(" "))
        vals.append([float(x) for x in f[1:]])
    return cols, ids, np.array(vals, dtype=np.float64).reshape(len(ids), len(cols))


def prepare(clust_path, gene_path, suffix=None):
    """The filters of :24-139 -> labels (the species row "-1" last), gene names, clust [K1 x S], genes [G x S]."""
    names, samples, ab = read_cluster_table(clust_path)
    kept = sorted((n[1:] if n.startswith("X") else n, k) for k, n in enumerate(names) if int((ab[:, k] > 0).sum()) >= 3)
    kept.sort(key=lambda t: (t[0].encode(), t[1]))
    if not kept:
        raise NoClusters()
    row_of = {}
    for s, name in enumerate(samples):
        if any(ab[s, k] > 0 for _, k in kept):
            row_of.setdefault(name, s)
    cols, ids, gv = read_gene_table(gene_path)
    use = []
    for attempt in ([""] if suffix is None else ["", suffix]):
        seen = set()
        for k, c in enumerate(cols):
            if c + attempt in row_of and c + attempt not in seen:
                seen.add(c + attempt)
                use.append((k, row_of[c + attempt]))
        if use:
            break
    if not use:
        raise ValueError("No overlapping sample IDs")
    gsel = gv[:, [k for k, _ in use]]
    keep = gsel.sum(axis=1) > 0
    genes = gsel[keep]
    gene_names = [i for i, k in zip(ids, keep) if k]
    rows = [s for _, s in use]
    clust = np.zeros((len(kept) + 1, len(use)))
    for i, (_, k) in enumerate(kept):
        v = ab[rows, k]
        clust[i] = np.where(v > 0, v, 0.0)
        clust[-1] += clust[i]
    return [lab for lab, _ in kept] + ["-1"], gene_names, clust, genes


def tables(labels, gene_names, corr, n_obs, stats=corr_stats):
    """The two tables' rows, cluster-major, from gene_correlations' arrays; `stats` computes the derived columns."""
    out = {}
    for method, key in (("pearson", "r"), ("spearman", "rho")):
        pos = [(c, g) for c in range(len(labels)) for g in range(len(gene_names)) if corr["valid"][c, g]]
        est = np.array([corr[key][c, g] for c, g in pos], dtype=np.float64)
        st = stats(method, est, n_obs)
        rows = []
        for i, (c, g) in enumerate(pos):
            w = {"gene": gene_names[g], "cluster": labels[c], "statistic": st["statistic"][i], "p": st["p_value"][i], "estimate": est[i],
                 "n_obs": n_obs, "q": st["q_value"][i]}
            if method == "pearson":
                w["lo"], w["hi"] = st["conf_low"][i], st["conf_high"][i]
            rows.append(w)
        out[method] = rows
    return out


def select_specific(pearson_rows, spearman_rows, min_obs=10, cutoff=0.05, max_bad=0.2, min_pearson=0.8, min_spearman=0.6):
    """selectSubspeciesSpecificGenes (:238-303) -> (species rows, cluster rows) of (gene, cluster, correlated, not correlated)."""
    groups = {}
    order = []
    for method, rows, lim in (("pearson", pearson_rows, min_pearson), ("spearman", spearman_rows, min_spearman)):
        for w in rows:
            key = (w["gene"], w["cluster"])
            if key not in groups:
                groups[key] = [True, True]
                order.append(w["cluster"]) if w["cluster"] not in order else None
            passes = w["estimate"] >= lim and w["q"] < cutoff and w["n_obs"] >= min_obs
            groups[key][0] = groups[key][0] and passes
            groups[key][1] = groups[key][1] and w["estimate"] < max_bad
    rank = {c: i for i, c in enumerate(order)}
    keys = sorted(groups, key=lambda k: (k[0].encode(), rank[k[1]]))
    species = [(g, c, groups[(g, c)][0], groups[(g, c)][1]) for g, c in keys if c == "-1" and groups[(g, c)][0]]
    species_genes = {g for g, _, _, _ in species}
    per_gene = {}
    for g, c in keys:
        if c != "-1":
            corr = groups[(g, c)][0] and g not in species_genes
            per_gene.setdefault(g, []).append((g, c, corr, groups[(g, c)][1]))
    clusters = []
    for g in sorted(per_gene, key=lambda x: x.encode()):
        gs = per_gene[g]
        if sum(x[2] for x in gs) >= 1 and sum(x[3] for x in gs) >= 1:
            clusters += [x for x in gs if x[2] != x[3]]
    return species, clusters


def run_files(clust_path, gene_path, suffix=None, corr=None, stats=corr_stats):
    """The four files' texts (spearman, pearson, clusterSpecificGenes, speciesSpecificGenes) and the counts.
    corr: gene_correlations' result to use instead of the model's own (the device's, so that its error in r is not
    amplified into the tails of p when the derived columns are compared)."""
    labels, gene_names, clust, genes = prepare(clust_path, gene_path, suffix)
    if corr is None:
        corr = gene_correlations(clust, genes)
    t = tables(labels, gene_names, corr, clust.shape[1], stats)
    species, clusters = select_specific(t["pearson"], t["spearman"])
    texts = {"spearman": table_text("spearman", t["spearman"]), "pearson": table_text("pearson", t["pearson"]),
             "clusterSpecificGenes": groups_text(clusters), "speciesSpecificGenes": groups_text(species)}
    counts = (len(labels) - 1, len(gene_names), clust.shape[1], len({g for g, _, _, _ in clusters}))
    return texts, counts, (labels, gene_names, clust, genes)
