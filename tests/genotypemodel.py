"""subpopr's writeGenotypeFreqs -> computeUniquePosPerCluster (src/subpopr/R/writeGenotypeFreqs.R:2-112, :195-277) restated in numpy: what
tests/test_gpu_genotype.py compares csrc/genotype_k.hip and csrc/genotype.cpp with, pinned on its own by tests/test_genotype_model.py.

R's rowMeans and mean() sum in long double: the means here are sequential numpy.longdouble sums in ascending column order (np.add.accumulate
keeps the order), rounded to double before they are compared.  Restated from reading the R code; no R was run."""
import numpy as np

assert np.finfo(np.longdouble).nmant == 63, "the model needs the x87 long double that R sums in"

OK, SINGLE, NO_POSITIONS, CLUSTER_MISSING, CUTOFF_BAD = range(5)


class DomainError(ValueError):
    pass


class FormatError(ValueError):
    pass


def cluster_means(rows, clust, k):
    """Per row: (mean over the non-NaN cells of the cluster's columns [double, NaN without one], NaN count, count of cells < 50, columns)."""
    cols = np.flatnonzero(clust == k)
    sub = rows[:, cols]
    nan = np.isnan(sub)
    total = np.add.accumulate(np.where(nan, 0.0, sub).astype(np.longdouble), axis=1)[:, -1]
    valid = (~nan).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (total / valid.astype(np.longdouble)).astype(np.float64)
        lt = (sub < 50.0).sum(axis=1)
    return mean, nan.sum(axis=1), lt, len(cols)


def genotype_rows(rows, clust, threshold=80.0, guard=1e-6):
    """rows [P x S] in 0..100 with NaN, clust [S] in 0..K.  Returns select, flip (uint32 [P], bit i - 1 = cluster i) and near (bool [P]: a
    mean difference within `guard` of the threshold)."""
    rows = np.asarray(rows, dtype=np.float64)
    clust = np.asarray(clust, dtype=np.int64)
    n_clusters = int(clust.max())
    p = rows.shape[0]
    stats = [cluster_means(rows, clust, k) for k in range(1, n_clusters + 1)]
    n_used = sum(s[3] for s in stats)
    all_na = sum(s[1] for s in stats)
    select, flip, near = np.zeros(p, dtype=np.uint32), np.zeros(p, dtype=np.uint32), np.zeros(p, dtype=bool)
    for i, (mean, na, lt, size) in enumerate(stats):
        ok = (na.astype(np.float64) / np.float64(size) < 0.2) & ((all_na - na).astype(np.float64) / np.float64(n_used - size) < 0.2)
        for j, other in enumerate(stats):
            if j == i:
                continue
            with np.errstate(invalid="ignore"):
                f = np.abs(mean - other[0])
            f[np.isnan(f)] = 0.0
            ok &= f > threshold
            near |= np.abs(f - threshold) <= guard
        select |= ok.astype(np.uint32) << np.uint32(i)
        flip |= (ok & (lt > (size - na) - lt)).astype(np.uint32) << np.uint32(i)
    return select, flip, near


def r_mean(x):
    x = np.asarray(x, dtype=np.longdouble)
    n = np.longdouble(len(x))
    s = np.add.accumulate(x)[-1] / n
    t = np.add.accumulate(x - s)[-1]
    return float(s + t / n)


def r_median(x):
    """median(x, na.rm = T) of the values given: None (NA) without one."""
    x = sorted(x)
    if not x:
        return None
    h = len(x) // 2
    return x[h] if len(x) % 2 else r_mean(x[h - 1:h + 1])


def fmt(v):
    return "NA" if v is None else "NaN" if v != v else "%.15g" % v


def clustering_text(pairs):
    return "clust\n" + "".join("%s\t%s\n" % (n, c) for n, c in pairs)


def parse_clustering(text):
    lines = text.split("\n")
    if lines[0] != "clust":
        raise FormatError("header")
    out = {}
    for ln in lines[1:]:
        if not ln:
            continue
        cells = ln.split("\t")
        if len(cells) != 2 or not cells[0] or not cells[1].lstrip("+-").isdigit() or cells[0] in out:
            raise FormatError(ln)
        out[cells[0]] = int(cells[1])
    return out


def genotype_files(clustering, freq, species, uniq_threshold=0.8):
    """clustering: the text of <species>_mann_clustering.tab; freq: (sample names, row labels, table [P x S] in 0..1 with NaN for -1).
    Returns (files: name -> text, info: the result fields of msnv_genotype_file)."""
    id_of = parse_clustering(clustering)
    names, labels, table = freq
    table = np.asarray(table, dtype=np.float64)
    if (table[~np.isnan(table)] > 1.0).any():
        raise DomainError("a cell above 1")
    table = table * 100.0
    used = [s for s, n in enumerate(names) if n in id_of and names.index(n) == s]
    ids = [id_of[names[s]] for s in used]
    clust_ids = list(dict.fromkeys(ids))
    n_clusters = len(clust_ids)
    info = {"n_clusters": n_clusters, "n_samples": len(used), "n_rows": table.shape[0], "n_positions": 0, "n_rechecked": 0, "n_correct": 0, "n_good": 0}
    log = species + "_hap_out.txt"
    if n_clusters <= 1:
        return {log: "Single cluster\n"}, dict(info, status=SINGLE)
    files = {log: "\n"}
    if max(clust_ids) < 1:
        files[log] += "No genotyping positions for  %s\n" % species
        return files, dict(info, status=NO_POSITIONS)
    if n_clusters > 32:
        raise DomainError("more than 32 clusters")
    clust = np.zeros(len(names), dtype=np.int64)
    for s, c in zip(used, ids):
        clust[s] = clust_ids.index(c) + 1
    select, flip, near = genotype_rows(table, clust, uniq_threshold * 100.0)
    info["n_rechecked"] = int(near.sum())
    mean_of, median_of = {}, {}
    for k, cid in enumerate(clust_ids):
        picked = np.flatnonzero(select >> np.uint32(k) & 1)
        if len(picked) == 0:
            files[log] += "No unique genotyping positions for species %s cluster %d (species has %d total clusters)\n" % (species, cid, n_clusters)
            continue
        flipped = (flip[picked] >> np.uint32(k) & 1).astype(bool)
        files["%s_%d_hap_positions.tab" % (species, cid)] = "posId\tflip\n" + "".join(
            "%d\t%s\t%s\n" % (g + 1, labels[p], "TRUE" if f else "FALSE") for g, (p, f) in enumerate(zip(picked, flipped)))
        info["n_positions"] += len(picked)
        data = np.where(flipped[:, None], 100.0 - table[picked], table[picked])
        cols = [[float(v) for v in data[:, s] if v == v] for s in used]
        mean_of[k] = [r_mean(c) if c else float("nan") for c in cols]
        median_of[k] = [r_median(c) for c in cols]
    if not mean_of:
        files[log] += "No genotyping positions for  %s\n" % species
        return files, dict(info, status=NO_POSITIONS)
    if len(mean_of) < n_clusters:
        files[log] += "At least one cluster is missing genotyping positions for  %s . Aborting, but this could be fixed.\n" % species
        return files, dict(info, status=CLUSTER_MISSING)
    bad, good, n_without = [], [], 0
    for a in range(len(used)):
        coll = [median_of[k][a] for k in range(n_clusters)]
        if None in coll:
            n_without += 1
            continue
        total = float(np.add.accumulate(np.asarray(coll, dtype=np.longdouble))[-1])
        (bad if total > 120.0 or total < 80.0 else good).append(a)
    if len(bad) > 0.15 * len(used):
        files[log] += "Cutoff is bad\n"
        files[log] += ("In  %d  out of  %d  samples,  the summed abundance of all clusters per sample is >120%% or < 80%%,  based on the frequencies of the "
                       "genotyping SNVs.\n" % (len(bad), len(used)))
        files[log] += "Samples with incoherent cluster abundance measured based on genotyping SNVs: \n"
        files[log] += "".join(names[used[a]] + "\n" for a in bad)
        return files, dict(info, status=CUTOFF_BAD)
    for a in good:
        coll = [median_of[k][a] for k in range(n_clusters)]
        info["n_correct"] += ids[a] == coll.index(max(coll)) + 1
    info["n_good"] = len(good)
    files[log] += ("Genotyping-based assignment of discovery samples to clusters was correct for %d samples. Determined any cluster assignment from genotyping "
                   "SNVs for %d out of %d samples. Of those samples without assignments: %d  had incoherect cluster assignments and %d lacked coverage of "
                   "genotyping SNVs.\n" % (info["n_correct"], len(good), len(used), len(bad), n_without))
    for which, cells in (("mean", mean_of), ("median", median_of)):
        files["%s_hap_freq_%s.tab" % (species, which)] = "\ti\n" + "".join(
            "%s\t%s\t%d\n" % (names[used[a]], fmt(cells[k][a]), cid) for k, cid in enumerate(clust_ids) for a in range(len(used)))
    return files, dict(info, status=OK)
