"""A plain numpy restatement of the clustering stage (include/msnv.h: msnv_pam_tasks, msnv_pred_strength, msnv_cluster_file; the product is
metasnv_amd/csrc/cluster.cpp + cluster_k.hip), for the tests: cluster::pam's BUILD and SWAP as the header words them, predStrengthCustom
(src/subpopr/R/clustering.R:152-216), computeClusters' sample selection, the stability of the cluster number and the files.

Every sum over j is sequential (np.add.accumulate(...)[-1] keeps the order; np.sum would add pairwise), R's mean() is in numpy.longdouble, and
the draws are the library's own generator.  The loops over candidates are vectorised, the order inside each sum is not touched."""
import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
MASK = (1 << 64) - 1
MAX_SWAPS = 65536


# ---- the draws
def mix(x):
    z = (x + 0x9e3779b97f4a7c15) & MASK
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def draw(seed, ordinal, i):
    return mix((mix((mix(seed & MASK) + ordinal) & MASK) + i) & MASK)


def permutation(seed, ordinal, n):
    p = list(range(n))
    for i in range(n - 1, 0, -1):
        j = draw(seed, ordinal, i) % (i + 1)
        p[i], p[j] = p[j], p[i]
    return p


def seqsum(a, axis=-1):
    """The sequential sum along an axis (0.0 for an empty one)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(a.shape[:-1])
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


# ---- cluster::pam(diss = TRUE), pamonce = 0
def pam(d, k):
    """d: the task's m x m sub-matrix.  Returns (medoids: ascending 0-based positions, cluster: 1..k per member, n_swaps)."""
    d = np.asarray(d, dtype=np.float64)
    m = d.shape[0]
    assert 1 <= k < m
    s = 1.1 * float(d.max()) + 1.0
    dysma = np.full(m, s)
    ismed = np.zeros(m, dtype=bool)
    for _ in range(k):                                         # BUILD
        beter = seqsum(np.maximum(dysma[None, :] - d, 0.0))    # beter[i] = sum_j (dysma[j] - d(i, j) where > 0); adding +0.0 changes nothing
        beter[ismed] = -1.0
        i = int(np.flatnonzero(beter == beter.max())[-1])      # the LAST largest (ammax <= beter[i])
        ismed[i] = True
        dysma = np.minimum(dysma, d[i])
    sky = float(seqsum(dysma))
    n_swaps = 0
    while k > 1:                                               # SWAP
        med = np.flatnonzero(ismed)
        dysma, dysmb = np.full(m, s), np.full(m, s)
        for i in med:                                          # ascending, strict comparisons
            first = dysma > d[i]
            second = ~first & (dysmb > d[i])
            dysmb = np.where(first, dysma, np.where(second, d[i], dysmb))
            dysma = np.where(first, d[i], dysma)
        hs = np.flatnonzero(~ismed)
        hj = d[hs][:, None, :]                                 # [h][.][j]
        ij = d[med][None, :, :]                                # [.][i][j]
        a, b = dysma[None, None, :], dysmb[None, None, :]
        contrib = np.where(ij == a, np.where(b > hj, hj, b) - a, np.where(hj < a, hj - a, 0.0))
        dz = seqsum(contrib)                                   # [h][i], each a sequential sum over j
        flat = dz.ravel()                                      # h ascending, then i ascending: the loop order
        best = int(np.argmin(flat))                            # the FIRST smallest
        dzsky = float(flat[best]) if flat[best] < 1.0 else 1.0
        if not dzsky < -16.0 * DBL_EPSILON * abs(sky):
            break
        n_swaps += 1
        if n_swaps > MAX_SWAPS:
            raise RuntimeError("pam: did not settle")
        h, i = hs[best // k], med[best % k]
        ismed[i], ismed[h] = False, True
        sky += dzsky
    med = np.flatnonzero(ismed)
    cluster = np.argmin(d[med], axis=0) + 1                    # nearest medoid, the first on ties
    return med.astype(np.int64), cluster.astype(np.int64), n_swaps


def cost(d, med):
    return float(np.min(np.asarray(d)[list(med)], axis=0).sum())


# ---- predStrengthCustom
def classify(d, members, medoids):
    """fpc::classifdist(method = "centroid"): which.min over the medoids' distances, so the first medoid on ties.  0-based cluster per member."""
    return np.argmin(np.asarray(d)[np.ix_(members, medoids)], axis=1)


def split_strength(d, order, k):
    """One (k, l): order = the samples (global indices) in the permutation's order; returns prederr[[k]][l]."""
    d = np.asarray(d, dtype=np.float64)
    order = np.asarray(order, dtype=np.int64)
    n = len(order)
    nf = (n // 2, n - n // 2)
    halves = (order[:nf[0]], order[nf[0]:])
    fits = [pam(d[np.ix_(h, h)], k) for h in halves]
    mins = []
    for i in (0, 1):
        other_medoids = halves[1 - i][fits[1 - i][0]]          # global indices, in cluster order
        cls = classify(d, halves[i], other_medoids)
        clus = fits[i][1]
        ps = []
        for kk in range(1, k + 1):
            nik = int((clus == kk).sum())
            if nik > 1:
                a = np.flatnonzero(clus[:nf[i] - 1] == kk)     # the half's last entry is left out of the numerator, not of nik
                same = int((cls[a][:, None] == cls[a][None, :]).sum())
                ps.append((same - len(a)) / (nik * (nik - 1)))
            else:
                ps.append(0.0)
        mins.append(min(ps))
    return (mins[0] + mins[1]) / 2.0


def r_mean(x):
    x = np.asarray(x, dtype=np.longdouble)
    n = np.longdouble(len(x))
    s = np.add.accumulate(x)[-1] / n
    t = np.add.accumulate(x - s)[-1]
    return float(s + t / n)


def r_sd(x):
    m = np.longdouble(r_mean(x))
    dev = np.asarray(x, dtype=np.longdouble) - m
    return float(np.sqrt(np.float64(np.add.accumulate(dev * dev)[-1] / np.longdouble(len(x) - 1))))


def summarise(prederr, cutoff):
    """prederr [k_max - 1][M] -> (mean_pred [k_max], optimalk)."""
    mean_pred = [1.0] + [r_mean(row) for row in prederr]
    optimalk = max(k + 1 for k, v in enumerate(mean_pred) if v > cutoff)
    return np.array(mean_pred), optimalk


def pred_strength(d, k_max, perms, cutoff=0.8):
    """perms [k_max - 1][M][n] of global indices.  Returns prederr, mean_pred, optimalk."""
    prederr = np.array([[split_strength(d, perms[k - 2][l], k) for l in range(len(perms[k - 2]))] for k in range(2, k_max + 1)])
    mean_pred, optimalk = summarise(prederr, cutoff)
    return prederr, mean_pred, optimalk


def max_clusters_to_try(n, default, min_size):
    return max(0, min(default, n // 2 - 1, n // min_size))


def run_strength(d, members, gmax, big_m, seed, ord_base, cutoff):
    """A whole prediction-strength run over `members` with the library's draws."""
    perms = [[[members[q] for q in permutation(seed, ord_base + (k - 2) * big_m + l, len(members))] for l in range(big_m)] for k in range(2, gmax + 1)]
    return pred_strength(d, gmax, perms, cutoff)


def stab_score(props, nums):
    """getNClusStabScore: nums holds None for NA.  1 Low, 2 Medium, 3 High."""
    def group(tenth):
        g = [v for p, v in zip(props, nums) if int(np.floor(p * 10.0 + 0.5)) == tenth]
        constant = len(g) >= 2 and None not in g and len(set(g)) == 1
        return constant, (g[0] if g else None)
    c100, n100 = group(10)
    if not c100:
        return 1
    (c90, n90), (c80, n80) = group(9), group(8)
    return 3 if (c90 and c80 and n90 == n100 and n80 == n100) else 2


def fmt(v):
    return "NaN" if v != v else "%.15g" % v


def dist_text(names, d, members):
    lines = ["\t".join(names[i] for i in members)]
    for i in members:
        lines.append(names[i] + "\t" + "\t".join(fmt(d[i, j]) for j in members))
    return "\n".join(lines) + "\n"


def freq_bands(col):
    """One sample column of the freq table (NaN = -1 / NA): the three proportions of computeSnvFreqStats."""
    x = col[~np.isnan(col)]
    with np.errstate(invalid="ignore", divide="ignore"):
        return [np.float64(((x < lo) | (x > hi)).sum()) / np.float64(len(x)) for lo, hi in ((20, 80), (10, 90), (5, 95))]


def cluster_files(names, d, species, freq=None, seed=1, ps_cut=0.8, stability_iters=10, big_m=50):
    """The stage.  names, d: the distance matrix; freq: (sample names, table [positions x samples] with NaN for -1) or None.
    Returns (files: path relative to the output directory -> text, info: status, n_clusters, n_samples, n_outliers, stability_score, optimalk)."""
    d = np.asarray(d, dtype=np.float64)
    n_all = len(names)
    prefix = species + "_mann"
    files, info = {}, {"stability_score": 0, "optimalk": 0, "n_clusters": 0}
    # removeOutliersFromDistMatrixMinDissim
    off = d + np.where(np.eye(n_all, dtype=bool), np.inf, 0.0)
    mind = off.min(axis=1)
    mean, sd = r_mean(mind), r_sd(mind)
    hi, lo = mean + 3 * sd, mean - 3 * sd
    keep = [i for i in range(n_all) if not (mind[i] > hi or mind[i] < lo)]
    qc = keep if 0 < n_all - len(keep) <= 5 else list(range(n_all))
    info["n_outliers"] = n_all - len(qc)
    used, composition = list(qc), None
    if freq is not None:
        fnames, table = freq
        composition = "freq_data_sample_20_80\tfreq_data_sample_10_90\tfreq_data_sample_5_95\n"
        used = []
        for s, name in enumerate(fnames):
            bands = freq_bands(np.asarray(table, dtype=np.float64)[:, s])
            composition += name + "\t" + "\t".join(fmt(float(v)) for v in bands) + "\n"
            cand = [i for i in qc if names[i] == name]
            if bands[1] >= 0.8 and cand and cand[0] not in used:
                used.append(cand[0])
        status = None
        if len(used) < 6:
            status = 3
        elif len({d[a, b] for ai, a in enumerate(used) for b in used[:ai]}) <= 1:
            status = 4
        if status is not None:
            files["clustMedoidDefnFailed/" + species + "_freq_composition.tab"] = composition
            info.update(status=status, n_samples=len(used))
            return files, info
    n = len(used)
    gmax = max_clusters_to_try(n, 15, 3)
    optimalk, mean_pred = 1, None
    if gmax > 1:
        _, mean_pred, optimalk = run_strength(d, used, gmax, big_m, seed, 0, ps_cut)
    _, clus, _ = pam(d[np.ix_(used, used)], optimalk)
    props, nums = [], []
    if n >= 10:
        low = max(0.3, np.ceil(10.0 / n * 10) / 10)
        pi = 0
        while low + pi * 0.1 <= 1 + 1e-10:
            prop = low + pi * 0.1
            size = min(n, int(np.floor(n * prop)))
            for it in range(stability_iters):
                r = 1 + 1024 * pi + it
                sub = [used[q] for q in permutation(seed, (r << 32) | 0xffffffff, n)[:size]]
                g = max_clusters_to_try(size, 10, 5)
                props.append(prop)
                nums.append(run_strength(d, sub, g, big_m, seed, r << 32, ps_cut)[2] if g > 1 else None)
            pi += 1
        info["stability_score"] = stab_score(props, nums)
    sizes = {c: int((clus == c).sum()) for c in range(1, optimalk + 1)}
    big = [c for c in sizes if sizes[c] >= 3]
    one = len(big) <= 1
    sub_dir = "noClustering/" if one else ""
    if gmax <= 1:
        files["clustMedoidDefnFailed/" + prefix + "_distMatrixUsedForClustMedoidDefns.txt"] = dist_text(names, d, used)
    else:
        files[sub_dir + prefix + "_PS_values.tab"] = "x\n" + "".join("%d\t%s\n" % (k + 1, fmt(float(v))) for k, v in enumerate(mean_pred))
    files[sub_dir + prefix + "_distMatrixUsedForClustMedoidDefns.txt"] = dist_text(names, d, used)
    if composition is not None:
        files[sub_dir + species + "_freq_composition.tab"] = composition
    files[sub_dir + prefix + "_clustering.tab"] = clustering_text([names[i] for i in qc], [1] * len(qc)) if one else \
        clustering_text([names[used[a]] for a in range(n) if sizes[clus[a]] >= 3], [int(clus[a]) for a in range(n) if sizes[clus[a]] >= 3])
    if props:
        files[sub_dir + prefix + "_clusNumStability.tab"] = "propSamples\tnumClusters\n" + "".join(
            "%s\t%s\n" % (fmt(p), "NA" if v is None else str(v)) for p, v in zip(props, nums))
    info.update(status=2 if gmax <= 1 else 1 if one else 0, n_clusters=1 if one else len(big), n_samples=n, optimalk=optimalk)
    return files, info


def clustering_text(samples, ids):
    """write.table(data.frame(clust = ...), sep = "\\t", quote = F): the header has no cell for the row names."""
    return "clust\n" + "".join("%s\t%d\n" % (s, c) for s, c in zip(samples, ids))
