"""subpopr's writeSubpopsForAllSamples (src/subpopr/R/writeSubpopsForAllSamples.R) and writeSubpopAbundSpeciesAbund (src/subpopr/R/writeSubpopAbund.R:
99-169) restated in numpy: what tests/test_gpu_profile.py compares csrc/profile_k.hip and csrc/profile.cpp with, pinned on its own by
tests/test_profile_model.py.

The order statistics come from np.sort; R's mean(), sd() and rowSums() sum in long double: sequential numpy.longdouble sums here (np.add.accumulate
keeps the order).  Restated from reading the R code; no R was run."""
import numpy as np

from genotypemodel import DomainError, FormatError, fmt, r_mean

assert np.finfo(np.longdouble).nmant == 63, "the model needs the x87 long double that R sums in"

OK, NO_FILES, NONE_USABLE = range(3)
SUMMARY_HEADER = "Sample\tCluster\tmean\tmedian\tstandardDeviation\tprevalence\tprevalenceGte5\tn0\tn100\tnNoCoverage\n"


def r_sd(x):
    """sd(): squared deviations from mean() (a double) summed in long double, over n - 1; None (NA) at n = 1."""
    if len(x) < 2:
        return None
    d = np.asarray(x, dtype=np.longdouble) - np.longdouble(r_mean(x))
    return float(np.sqrt(np.float64(np.add.accumulate(d * d)[-1] / np.longdouble(len(x) - 1))))


def long_sum(x):
    return float(np.add.accumulate(np.asarray(x, dtype=np.longdouble))[-1])


def flipped(rows, flip):
    """The matrix as the statistics see it: flipped rows as 100 - x, -0.0 as +0.0."""
    rows = np.asarray(rows, dtype=np.float64) + 0.0
    return np.where(np.asarray(flip, dtype=bool)[:, None], 100.0 - rows, rows)


def profile_columns(rows, flip):
    """rows [G x S] in 0..100 with NaN, flip [G].  Returns a dict of arrays over the columns: n_called, n_gt0, n_ge5, n_eq0, n_eq100 and mid_lo, mid_hi
    (the called cells' order statistics of ranks (n - 1) // 2 and n // 2; NaN at n = 0)."""
    data = flipped(rows, flip)
    if ((data < 0.0) | (data > 100.0)).any():
        raise DomainError("a cell outside [0, 100]")
    s = data.shape[1]
    out = {k: np.zeros(s, dtype=np.uint32) for k in ("n_called", "n_gt0", "n_ge5", "n_eq0", "n_eq100")}
    out["mid_lo"], out["mid_hi"] = np.full(s, np.nan), np.full(s, np.nan)
    for c in range(s):
        x = np.sort(data[:, c][~np.isnan(data[:, c])])
        n = len(x)
        out["n_called"][c], out["n_gt0"][c], out["n_ge5"][c] = n, (x > 0).sum(), (x >= 5).sum()
        out["n_eq0"][c], out["n_eq100"][c] = (x == 0).sum(), (x == 100).sum()
        if n:
            out["mid_lo"][c], out["mid_hi"][c] = x[(n - 1) // 2], x[n // 2]
    return out


def freq_id(i):
    f = i.split(":")
    if len(f) < 4:
        raise FormatError(i)
    return ":".join((f[0], f[2], f[3]))


def hap_id(i):
    """contig:ann:pos:T>A:. -> contig:pos:A (sub('.>', '', x): the first '>' with the character before it)."""
    f = i.split(":")
    if len(f) < 4:
        raise FormatError(i)
    base = f[3]
    gt = base.find(">", 1)
    if gt >= 0:
        base = base[:gt - 1] + base[gt + 1:]
    return ":".join((f[0], f[2], base))


def cluster_files(species, names):
    """The names <species>_*.pos.freq among `names`, in byte order."""
    return sorted((n for n in names if n.startswith(species + "_") and n.endswith(".pos.freq")), key=lambda n: n.encode())


def cluster_number(name):
    spec_hap = name.split(".")[0]
    tail = spec_hap.rsplit("_", 1)[-1]
    if "_" not in spec_hap or not tail.lstrip("+-").isdigit() or len(tail.lstrip("+-")) > 9 or tail[1:2] in ("+", "-"):
        raise FormatError(name)
    return spec_hap, int(tail)


def sample_names(all_samples_text):
    out = []
    for ln in all_samples_text.split("\n"):
        tok = ln.split()
        if tok and not tok[0].startswith("#"):
            out.append(tok[0].rstrip("/").rsplit("/", 1)[-1])
    return out


def read_cluster(freq_text, hap_text, n_samples, path="file"):
    """The G x S matrix in the order of the positions file and its flips."""
    row_of, cells = {}, []
    for ln in freq_text.split("\n"):
        if not ln:
            continue
        f = ln.split("\t")
        if len(f) != n_samples + 1:
            raise FormatError("File: %s does not have expected number of columns (each column is a sample). According to all_samples, it should have %d columns."
                              % (path, n_samples))
        i = freq_id(f[0])
        if i in row_of:
            raise FormatError("duplicate " + i)
        row_of[i] = len(cells)
        cells.append([np.nan if float(v) == -1 else float(v) for v in f[1:]])
    lines = [ln for ln in hap_text.split("\n") if ln]
    if lines[0] != "posId\tflip":
        raise FormatError("header")
    rows, flip, seen = [], [], set()
    for ln in lines[1:]:
        f = ln.split("\t")
        if len(f) != 3 or f[2] not in ("TRUE", "FALSE"):
            raise FormatError(ln)
        i = hap_id(f[1])
        if i in seen:
            raise FormatError("duplicate " + i)
        seen.add(i)
        rows.append(cells[row_of[i]] if i in row_of else [np.nan] * n_samples)
        flip.append(f[2] == "TRUE")
    return np.array(rows, dtype=np.float64).reshape(len(rows), n_samples), np.array(flip, dtype=bool)


def summarise(rows, flip, max_prop_uncalled):
    """The kept columns of one cluster: (column, mean, median, sd, prevalence, prevalenceGte5, n0, n100, nNoCoverage) each."""
    g = rows.shape[0]
    col = profile_columns(rows, flip)
    data = flipped(rows, flip)
    out = []
    for c in range(rows.shape[1]):
        n = int(col["n_called"][c])
        if not np.float64(n) >= np.float64(max_prop_uncalled) * np.float64(g):
            continue
        x = [float(v) for v in data[:, c] if v == v]
        out.append((c, r_mean(x), r_mean([col["mid_lo"][c], col["mid_hi"][c]]), r_sd(x), float(np.float64(col["n_gt0"][c]) / np.float64(n)),
                    float(np.float64(col["n_ge5"][c]) / np.float64(n)), int(col["n_eq0"][c]), int(col["n_eq100"][c]), g - n))
    return out


def stat_none_usable(species, n):
    return "Species %s: 0/%d clusters had usable placing data.\n" % (species, n)


def stat_incoherent(species, n_full, n_low, n_multi):
    return ("Species %s: %d out of %d samples rejected due to incoherent subpecies assignment. Number of samples where summed abundance of clusters was < 80%%: %d. "
            "Number of samples where summed abundance of clusters was > 120%%:%d\n" % (species, n_low + n_multi, n_full, n_low, n_multi))


def stat_bad(species, n_bad, n_coherent):
    return ("Species %s: %d out of %d samples rejected due to extreme mismatch between median abundance of genotyping SNVs (>30%%) and prevalence of genotyping SNVs "
            "(<75%%).\n" % (species, n_bad, n_coherent))


def wide_table(header, names, rows):
    return "\t".join(str(h) for h in header) + "\n" + "".join(n + "\t" + "\t".join(fmt(v) for v in r) + "\n" for n, r in zip(names, rows))


def clustering_table(names, rows, min_genotype_abundance=80.0):
    out = "clust\n"
    for n, r in zip(names, rows):
        above = [k + 1 for k, v in enumerate(r) if v > min_genotype_abundance]
        out += "%s\t%s\n" % (n, above[0] if len(above) == 1 else "NA")
    return out


def profile_files(species, all_samples_text, tree, max_prop_uncalled=0.2, min_genotype_abundance=80.0):
    """tree: file name -> text, the directory's content.  Returns (files: name -> text written, <species>_extended_clustering_stat.txt holding what is
    appended; info: the result fields of msnv_subpop_profile_files).  The two cases the reference cannot handle raise DomainError with .files = what
    was written before."""
    if not (0.0 < max_prop_uncalled <= 1.0):
        raise DomainError("max_prop_uncalled")
    samples = sample_names(all_samples_text)
    found = cluster_files(species, tree)
    pre = species + "_extended_clustering"
    info = dict(status=OK, n_files=len(found), n_usable=0, n_full=0, n_filtered=0, n_incoherent=0, n_bad=0, n_assigned=0)
    if not found:
        return {pre + "_stat.txt": stat_none_usable(species, 0)}, dict(info, status=NO_FILES)
    usable = []
    for name in found:
        spec_hap, number = cluster_number(name)
        rows, flip = read_cluster(tree[name], tree[spec_hap + "_hap_positions.tab"], len(samples), name)
        kept = summarise(rows, flip, max_prop_uncalled) if len(rows) else []
        if len(kept) >= 2:
            usable.append((number, kept))
    info["n_usable"] = len(usable)
    if not usable:
        return {pre + "_stat.txt": stat_none_usable(species, len(found))}, dict(info, status=NONE_USABLE)
    files = {pre + "_abundanceSummaryStats.tsv": SUMMARY_HEADER + "".join(
        "%s\t%d\t%s\t%d\t%d\t%d\n" % (samples[r[0]], number, "\t".join(fmt(v) for v in r[1:6]), r[6], r[7], r[8]) for number, kept in usable for r in kept)}
    full = [s for s in range(len(samples)) if all(any(r[0] == s for r in kept) for _, kept in usable)]
    if 1 not in [number for number, _ in usable] or not full:
        err = DomainError("cluster 1 is not usable" if full else "no sample in every cluster")
        err.files = files
        raise err
    med = [[next(r[2] for r in kept if r[0] == s) for _, kept in usable] for s in full]
    bad = {r[0] for _, kept in usable for r in kept if r[2] > 30.0 and r[4] < 0.75}
    sums = [long_sum(m) for m in med]
    n_low, n_multi = sum(t < 80.0 for t in sums), sum(t > 120.0 for t in sums)
    coherent = [i for i, t in enumerate(sums) if 80.0 <= t <= 120.0]
    stat = ""
    if n_low + n_multi:
        stat += stat_incoherent(species, len(full), n_low, n_multi)
    if bad:
        stat += stat_bad(species, len(bad), len(coherent))
    filtered = [i for i in coherent if full[i] not in bad]
    header = [number for number, _ in usable]
    if stat:
        files[pre + "_stat.txt"] = stat
    files[pre + "_wFreq_unfiltered.tab"] = wide_table(header, [samples[s] for s in full], med)
    files[pre + "_wFreq.tab"] = wide_table(header, [samples[full[i]] for i in filtered], [med[i] for i in filtered])
    files[pre + ".tab"] = clustering_table([samples[full[i]] for i in filtered], [med[i] for i in filtered], min_genotype_abundance)
    n_assigned = sum(not ln.endswith("\tNA") for ln in files[pre + ".tab"].split("\n")[1:] if ln)
    return files, dict(info, n_full=len(full), n_filtered=len(filtered), n_incoherent=n_low + n_multi, n_bad=len(bad), n_assigned=n_assigned)


def r_make_name(n):
    n = "".join(c if c.isalnum() or c in "._" else "." for c in n)
    ok = n and (n[0].isalpha() or (n[0] == "." and not n[1:2].isdigit()))
    return n if ok else "X" + n


def abundance_files(species, wfreq_text, abundance_text, sample_suffix=None):
    """Returns (files: name -> text, counts: samples used, clusters, samples in wFreq.tab, sample columns of the abundance table)."""
    lines = [ln for ln in wfreq_text.split("\n") if ln]
    cnames = [r_make_name(n) for n in lines[0].split("\t")]
    fsamples = [ln.split("\t")[0] for ln in lines[1:]]
    freq = [[float(v) for v in ln.split("\t")[1:]] for ln in lines[1:]]
    table = [ln.split("#")[0] for ln in abundance_text.split("\n")]
    table = [ln.split("\t") for ln in table if ln.strip(" \t")]
    tnames = table[0][1:]
    match = [r for r in table[1:] if r[0] == species]
    if not match:
        raise DomainError("Species not found in the species abundance profile. Species: " + species)
    if len(match) > 1:
        raise DomainError("More than one species in the abundance profile matched for species named: " + species)
    if not fsamples:
        raise DomainError("Species does not have cluster frequencies. Species: " + species)
    use = []
    for suffix in ("",) if sample_suffix is None else ("", sample_suffix):
        seen = set()
        for c, n in enumerate(tnames):
            if n + suffix in fsamples and n + suffix not in seen:
                seen.add(n + suffix)
                use.append((c, fsamples.index(n + suffix)))
        if use:
            break
    if not use:
        raise DomainError("No overlapping sample IDs between clustering and apecies abundance profiles. Are IDs formatted differently? Example clustering IDs: %s. "
                          "Example species profile IDs:%s" % (", ".join(fsamples[-3:]), ", ".join(tnames[-3:])))
    abund = [float(match[0][c + 1]) for c, _ in use]
    out = [[float(np.float64(v) / np.float64(100.0) * np.float64(a)) for v in freq[r]] for (_, r), a in zip(use, abund)]
    names = [fsamples[r] for _, r in use]
    files = {species + "_allClust_relativeAbund.tab": wide_table(cnames, names, out)}
    for k in range(len(cnames)):
        files["%s_clust_%d_hap_coverage_extended_normed.tab" % (species, k + 1)] = wide_table(cnames[k:k + 1], names, [r[k:k + 1] for r in out])
    return files, (len(use), len(cnames), len(fsamples), len(tnames))
