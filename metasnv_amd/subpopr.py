"""subpopr's two raw-SNV consumers, same argv and the same files as the reference scripts:

  getGenotypingSNVSubset.py <hapDir> <metaSNVdir>     (src/subpopr/inst/getGenotypingSNVSubset.py)
      <hapDir>/*hap_positions.tab + <metaSNVdir>/snpCaller/called_SNPs*  ->  <hapDir>/<species>.pos
  convertSNVtoAlleleFreq.py <file.pos> <minDepth>     (src/subpopr/inst/convertSNVtoAlleleFreq.py)
      <file.pos>  ->  <file.pos>.freq

  correlateSubpopProfileWithGeneProfiles.py <species> <outDir> <geneAbundanceFile> <geneFamilyType> [--sample-suffix S]
      (src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R, the function's argument order)
      <outDir>/<species>_allClust_relativeAbund.tab + the gene-family table  ->  <outDir>/<species>_corr<type>-{spearman,pearson,
      clusterSpecificGenes,speciesSpecificGenes}.tsv

  clusterSubpops.py <dist_file> <outDir> [--freq FILE] [--seed N] [--ps-cut X]
      (src/subpopr/R/clustering.R computeClusters with its defaults; species = the dist file's name up to its first '.')
      <species>.filtered.mann.dist (+ <species>.filtered.freq)  ->  <outDir>[/noClustering|/clustMedoidDefnFailed]/<species>_mann_{PS_values.tab,
      distMatrixUsedForClustMedoidDefns.txt,clustering.tab,clusNumStability.tab} and <species>_freq_composition.tab

  pcoaSubpops.py <dist_file> <dir> [--species S]
      (src/subpopr/R/clustering.R computePCoA: ape::pcoa of the matrix after outlier removal; <dir> = clusterSubpops.py's outDir or its noClustering/)
      <species>.filtered.mann.dist + <dir>/<species>_mann_clustering.tab (+ <species>_freq_composition.tab)  ->  <dir>/<species>_mann_pcoa_proj.tab
      and, our own file, <species>_mann_pcoa_eig.tab

  heatmapSubpops.py <dist_file> <dir> [--species S]
      (src/subpopr/inst/rmd/detailedSpeciesReport.rmd:142, :222, :250, :402: the row order of the distance heatmaps, hclust + reorder.dendrogram)
      <species>.filtered.mann.dist (+ <dir>/<species>_mann_distMatrixUsedForClustMedoidDefns.txt, _clustering.tab)  ->  our own files
      <dir>/<species>_mann_{hclust,heatmap}_{all,discovery}.tab

  snvFreqSubpops.py <freq_file> <outDir> [--species S] [--fix-read-threshold X] [--fix-snv-threshold Y]
      (src/subpopr/R/snvFreqPlot.R snvFreqPlot, the first step of defineSubpopulations, with computeClusters' strict band beside it)
      <species>.filtered.freq  ->  our own files <outDir>/snvFreqPlots/<species>_snvFreq_{cutoffs,fixed}.tab

  clusterMembStability.py <species> <dir> [--k N] [--ps-cut X] [--seed N] [--boot N]
      (src/subpopr/R/clusteringStability.R getClusMembStability and getClusMembStabScore; <dir> = clusterSubpops.py's outDir or its noClustering/)
      <dir>/<species>_mann_distMatrixUsedForClustMedoidDefns.txt (+ _PS_values.tab, _clusNumStability.tab)  ->  <dir>/<species>_mann_{clusMembStability.tab,
      stabilityAssessment.tab}

  summariseClustering.py <outDir>
      (src/subpopr/R/summariseClusteringResults.R summariseClusteringResultsForAll, from the files above instead of the .rds; host only)
      ->  <outDir>/summary_clustering.csv

  writeGenotypeFreqs.py <species> <clustering.tab> <freq_file> <outDir> [--uniq-threshold X]
      (src/subpopr/R/writeGenotypeFreqs.R writeGenotypeFreqs with computeUniquePosPerCluster)
      <species>_mann_clustering.tab + <species>.filtered.freq  ->  <outDir>/<species>_<cluster>_hap_positions.tab, <species>_hap_out.txt and
      <species>_hap_freq_{mean,median}.tab

  profileSubpops.py <species> <metaSNVdir> <outDir> [--max-prop-uncalled X] [--min-genotype-abundance X]
      (src/subpopr/R/profileSubpops.R useGenotypesToProfileSubpops with writeSubpopsForAllSamples.R)
      <metaSNVdir>/all_samples + <outDir>/<species>_<cluster>.pos.freq + <species>_<cluster>_hap_positions.tab  ->
      <outDir>/<species>_extended_clustering_{abundanceSummaryStats.tsv,wFreq_unfiltered.tab,wFreq.tab,stat.txt} and <species>_extended_clustering.tab

  writeSubpopAbund.py <species> <outDir> <speciesAbundanceFile> [--sample-suffix S]
      (src/subpopr/R/writeSubpopAbund.R writeSubpopAbundSpeciesAbund; the mOTU variant is not built)
      <outDir>/<species>_extended_clustering_wFreq.tab + a species x samples abundance table  ->  <outDir>/<species>_allClust_relativeAbund.tab and
      <species>_clust_<x>_hap_coverage_extended_normed.tab

getGenotypingSNVSubset.py and writeSubpopAbund.py are text filters (native, no device work) and summariseClustering.py reads and writes small
tables in Python; the frequencies of convertSNVtoAlleleFreq.py, the correlations, every PAM run of clusterSubpops.py and clusterMembStability.py
with the matching of the re-clustered subsets, pcoaSubpops.py's centring and eigendecomposition, heatmapSubpops.py's agglomerations,
snvFreqSubpops.py's class counts per sample, writeGenotypeFreqs.py's walk over the frequency table and profileSubpops.py's counts and medians per
sample are computed on the GPU (msnv_snv_allele_freq, msnv_gene_corr, msnv_corr_stats, msnv_pam_tasks, msnv_pred_strength, msnv_cluster_boot,
msnv_pcoa, msnv_hclust_tasks, msnv_freq_curves, msnv_genotype_rows, msnv_subpop_profile_columns) and there is no CPU fallback for them."""
import ctypes as C
import glob
import os
import sys


def _paths(lst):
    arr = (C.c_char_p * len(lst))(*[p.encode() for p in lst])
    return arr, len(lst)


def genotyping_subset(hap_paths, snp_paths, out_dir):
    """The lists are read in the order given; returns (#distinct positions wanted, #lines written)."""
    from ._lib import lib, check
    h, nh = _paths(hap_paths)
    s, ns = _paths(snp_paths)
    npos, nl = C.c_uint64(), C.c_uint64()
    check(lib.msnv_genotyping_subset(h, nh, s, ns, out_dir.encode(), C.byref(npos), C.byref(nl)))
    return npos.value, nl.value


def get_genotyping_snv_subset_main(argv=None):                 # getGenotypingSNVSubset.py:5-48
    argv = sys.argv[1:] if argv is None else argv
    hap_dir, metasnv_dir = argv[0], argv[1]
    print("Getting subspecies genotyping info from: " + hap_dir + '/*hap_positions.tab')
    print("Getting SNV for all data from raw SNV calls: " + metasnv_dir + '/snpCaller/called_SNPs*')
    haps = glob.glob(hap_dir + '/*hap_positions.tab')          # directory order, like the reference
    snps = glob.glob(metasnv_dir + '/snpCaller/called_SNPs*')
    if len(haps) < 1:
        sys.exit("Error: no *hap_positions.tab files")
    if len(snps) < 1:
        sys.exit("Error: no /snpCaller/called_SNPs* files in metaSNV output directory")
    from ._lib import MsnvError, EDOMAIN
    try:
        genotyping_subset(haps, snps, hap_dir)
    except MsnvError as e:
        if e.code == EDOMAIN:
            sys.exit("Error: no parse-able data in " + hap_dir + "/*hap_positions.tab files")
        sys.exit("Error: {}".format(e))


def snv_allele_freq(ctx, pos_path, min_depth):
    """Writes pos_path + '.freq'; returns (#allele rows, kernel ms)."""
    from ._lib import lib, check
    n, ms = C.c_uint64(), C.c_double()
    check(lib.msnv_snv_allele_freq(ctx._h, pos_path.encode(), int(min_depth), C.byref(n), C.byref(ms)))
    return n.value, ms.value


def convert_snv_to_allele_freq_main(argv=None):                # convertSNVtoAlleleFreq.py:3-27
    argv = sys.argv[1:] if argv is None else argv
    pos_path, min_depth = argv[0], int(argv[1])
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        snv_allele_freq(ctx, pos_path, min_depth)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def gene_correlations(ctx, clust, genes):
    """clust [K1 x S] (the caller appends the species row), genes [G x S], already cut to the samples and genes in use.
    Returns rho, r, valid [K1 x G], the pseudocount and the kernels' ms (msnv_gene_corr)."""
    import numpy as np
    from ._lib import lib, check
    clust = np.ascontiguousarray(clust, dtype=np.float64)
    genes = np.ascontiguousarray(genes, dtype=np.float64)
    if clust.ndim != 2 or genes.ndim != 2 or clust.shape[1] != genes.shape[1]:
        raise ValueError("gene_correlations: clust [K1 x S] and genes [G x S] must share S")
    k1, s = clust.shape
    g = genes.shape[0]
    rho, r = np.empty((k1, g)), np.empty((k1, g))
    valid = np.empty((k1, g), dtype=np.uint8)
    pc, ms = C.c_double(), C.c_double()
    check(lib.msnv_gene_corr(ctx._h, k1, g, s, _dptr(clust), _dptr(genes), _dptr(rho), _dptr(r), valid.ctypes.data_as(C.POINTER(C.c_uint8)),
                             C.byref(pc), C.byref(ms)))
    return {"rho": rho, "r": r, "valid": valid.astype(bool), "pseudocount": pc.value, "ms_kernel": ms.value}


def corr_stats(ctx, method, estimate, n_obs):
    """cor.test's derived columns and BH q-values of one table (msnv_corr_stats); method 'pearson' or 'spearman'; n_obs a number or one per row.
    Returns statistic, p_value, q_value and, for pearson, conf_low / conf_high (NaN at 3 observations)."""
    import numpy as np
    from ._lib import lib, check, CORR_PEARSON, CORR_SPEARMAN
    m = {"pearson": CORR_PEARSON, "spearman": CORR_SPEARMAN}[method]
    est = np.ascontiguousarray(estimate, dtype=np.float64).ravel()
    n = est.size
    nobs = np.ascontiguousarray(np.broadcast_to(np.asarray(n_obs, dtype=np.int32), (n,)))
    out = {k: np.empty(n) for k in ("statistic", "p_value", "q_value")}
    lo = hi = None
    if m == CORR_PEARSON:
        out["conf_low"], out["conf_high"] = np.empty(n), np.empty(n)
        lo, hi = _dptr(out["conf_low"]), _dptr(out["conf_high"])
    check(lib.msnv_corr_stats(ctx._h, m, n, _dptr(est), nobs.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(out["statistic"]), _dptr(out["p_value"]),
                              lo, hi, _dptr(out["q_value"])))
    return out


def gene_corr_files(ctx, clust_abund_path, gene_abund_path, out_prefix, sample_suffix=None):
    """Writes out_prefix + '-spearman.tsv', '-pearson.tsv', '-clusterSpecificGenes.tsv', '-speciesSpecificGenes.tsv';
    returns (clusters tested, genes kept, samples used, specific genes) -- all 0, nothing written, when no cluster is seen in 3 samples."""
    from ._lib import lib, check
    counts = (C.c_uint64 * 4)()
    check(lib.msnv_gene_corr_files(ctx._h, clust_abund_path.encode(), gene_abund_path.encode(),
                                   None if sample_suffix is None else sample_suffix.encode(), out_prefix.encode(), counts))
    return tuple(counts)


def correlate_gene_profiles_main(argv=None):                   # correlateSubpopProfileWithGeneProfiles.R:3-227
    argv = list(sys.argv[1:] if argv is None else argv)
    suffix = None
    if "--sample-suffix" in argv:
        i = argv.index("--sample-suffix")
        if i + 1 >= len(argv):
            sys.exit("ERROR: --sample-suffix needs a value")
        suffix = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) != 4:
        sys.exit("usage: correlateSubpopProfileWithGeneProfiles.py SPECIES OUTDIR GENE_ABUNDANCE_FILE GENE_FAMILY_TYPE [--sample-suffix S]")
    species, out_dir, gene_path, family_type = argv
    clust_path = os.path.join(out_dir, species + "_allClust_relativeAbund.tab")
    if not os.path.exists(clust_path):                         # :7-13
        print("No cluster abundances file for species " + species + ". May be due to failed genotyping. "
              "Missing required file for gene content calculation: " + clust_path)
        return 0
    if not os.path.exists(gene_path):                          # :15-19
        print("Missing required gene abundances file for gene content calculation:  " + gene_path)
        return 0
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        k, g, s, n = gene_corr_files(ctx, clust_path, gene_path, os.path.join(out_dir, species + "_corr" + family_type), suffix)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    if k == 0:
        print("No subspecies seen in >= 3 samples for species:" + species)      # :32
        return 0
    print("Species " + species + ": Testing " + str(k) + " clusters for correlation with " + str(g) + " geneFamily groups in " + str(s) + " samples")   # :119-121
    if n == 0:
        print("No cluster-specific genes found for species " + species)         # :214
    return n


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def pam_tasks(ctx, dist, tasks):
    """cluster::pam(diss = TRUE) of many index subsets of dist [n x n] in one launch (msnv_pam_tasks).  tasks: (indices, k) pairs.
    Returns one dict per task: medoids (0-based positions in the task's list, ascending), cluster (1..k per list entry), n_swaps; and the kernel's ms."""
    import numpy as np
    from ._lib import lib, check
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError("pam_tasks: dist must be a square matrix")
    lists = [np.asarray(ix, dtype=np.int32).ravel() for ix, _ in tasks]
    m = np.array([len(x) for x in lists], dtype=np.int32)
    k = np.array([kk for _, kk in tasks], dtype=np.int32)
    idx = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32), dtype=np.int32)
    med = np.zeros(max(int(k.clip(min=0).sum()), 1), dtype=np.int32)
    clus = np.zeros(max(idx.size, 1), dtype=np.int32)
    swaps = np.zeros(max(len(tasks), 1), dtype=np.int32)
    ms = C.c_double()
    check(lib.msnv_pam_tasks(ctx._h, dist.shape[0], _dptr(dist), len(tasks), _iptr(m), _iptr(k), _iptr(idx), _iptr(med), _iptr(clus), _iptr(swaps), C.byref(ms)))
    out, o, mo = [], 0, 0
    for t in range(len(tasks)):
        out.append({"medoids": med[mo:mo + k[t]].copy(), "cluster": clus[o:o + m[t]].copy(), "n_swaps": int(swaps[t])})
        o += m[t]
        mo += k[t]
    return out, ms.value


def prediction_strength(ctx, dist, k_max, perms, cutoff=0.8):
    """predStrengthCustom for given permutations (msnv_pred_strength): perms [k_max - 1][M][n], one permutation of 0..n-1 per (k, l).
    Returns prederr [k_max - 1][M], mean_pred [k_max] (entry 0 is k = 1: 1.0), optimalk and the kernels' ms."""
    import numpy as np
    from ._lib import lib, check
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    perms = np.ascontiguousarray(perms, dtype=np.int32)
    n = dist.shape[0]
    if dist.ndim != 2 or dist.shape[1] != n or perms.ndim != 3 or perms.shape[0] != k_max - 1 or perms.shape[2] != n:
        raise ValueError("prediction_strength: dist [n x n], perms [k_max - 1][M][n]")
    big_m = perms.shape[1]
    prederr = np.empty((k_max - 1, big_m))
    mean_pred = np.empty(k_max)
    ok, ms = C.c_int32(), C.c_double()
    check(lib.msnv_pred_strength(ctx._h, n, _dptr(dist), k_max, big_m, _iptr(perms), float(cutoff), _dptr(prederr), _dptr(mean_pred), C.byref(ok), C.byref(ms)))
    return {"prederr": prederr, "mean_pred": mean_pred, "optimalk": ok.value, "ms_kernel": ms.value}


CLUSTER_REASONS = {                                            # what computeClusters returns instead of a table (clustering.R:64-74, :314)
    2: "Cluster medoid definition failed",
    3: "After removing samples that do not have extreme SNV frequencies, insufficient samples (< 6) remain to pick the number of clusters and cluster medoids.",
    4: "After removing samples that do not have extreme SNV frequencies, all values in the distance matrix are equivalent.",
}


def cluster_file(ctx, dist_path, out_dir, species=None, freq_path=None, seed=None, ps_cut=None, stability_iters=None, max_prop_reads_non_homog=None,
                 min_prop_homog_snv=None):
    """The stage on files (msnv_cluster_file_ex; subpopr's -x / -y as max_prop_reads_non_homog / min_prop_homog_snv, None: 0.1 / 0.8).  Returns a
    dict: status (_lib.CLUSTER_*), n_clusters, n_samples, n_outliers, stability_score (1 Low, 2 Medium, 3 High, 0 not rated), optimalk,
    n_pam_tasks, ms_kernel."""
    from ._lib import lib, check, ClusterOpts, ClusterFilter
    if species is None:
        species = os.path.basename(dist_path).split(".")[0]
    o = ClusterOpts()
    lib.msnv_cluster_opts_default(C.byref(o))
    if seed is not None:
        o.seed = int(seed)
    if ps_cut is not None:
        o.ps_cut = float(ps_cut)
    if stability_iters is not None:
        o.stability_iters = int(stability_iters)
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    flt = None
    if max_prop_reads_non_homog is not None or min_prop_homog_snv is not None:
        flt = ClusterFilter()
        lib.msnv_cluster_filter_default(C.byref(flt))
        if max_prop_reads_non_homog is not None:
            flt.max_prop_reads_non_homog = float(max_prop_reads_non_homog)
        if min_prop_homog_snv is not None:
            flt.min_prop_homog_snv = float(min_prop_homog_snv)
    check(lib.msnv_cluster_file_ex(ctx._h, dist_path.encode(), None if freq_path is None else freq_path.encode(), species.encode(), out_dir.encode(),
                                   C.byref(o), None if flt is None else C.byref(flt), res, C.byref(ms)))
    return {"status": res[0], "n_clusters": res[1], "n_samples": res[2], "n_outliers": res[3], "stability_score": res[4], "optimalk": res[5],
            "n_pam_tasks": res[6], "ms_kernel": ms.value}


def cluster_subpops_main(argv=None):                           # clustering.R:20-133 computeClusters
    import argparse
    ap = argparse.ArgumentParser(prog="clusterSubpops.py", description="Cluster a species' samples into subspecies (subpopr's computeClusters) on the GPU.")
    ap.add_argument("dist_file", metavar="DIST_FILE", help="<species>.filtered.mann.dist of metaSNV_DistDiv.py --dist")
    ap.add_argument("out_dir", metavar="OUTDIR")
    ap.add_argument("--freq", metavar="FILE", help="<species>.filtered.freq: keep only samples with extreme SNV frequencies")
    ap.add_argument("--seed", type=int, default=None, metavar="N")
    ap.add_argument("--ps-cut", type=float, default=None, metavar="X", help="prediction-strength cutoff (0.8)")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    for f in (a.dist_file, a.freq):
        if f is not None and not os.path.exists(f):
            sys.exit("ERROR: missing input file: " + f)
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = cluster_file(ctx, a.dist_file, a.out_dir, freq_path=a.freq, seed=a.seed, ps_cut=a.ps_cut)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    species = os.path.basename(a.dist_file).split(".")[0]
    if res["status"] in CLUSTER_REASONS:
        print("Species " + species + ": " + CLUSTER_REASONS[res["status"]])
    else:
        print("Species " + species + ": " + str(res["n_clusters"]) + " cluster(s) from " + str(res["n_samples"]) + " samples; cluster number stability: "
              + ("not rated", "Low", "Medium", "High")[res["stability_score"]])
    return res


def pcoa(ctx, dist, n_axes=2):
    """ape::pcoa(correction = "none") of dist [n x n] by the device's Jacobi solver (msnv_pcoa).  Returns a dict: eig, rel_eig, axis_pct
    (float64 [n], descending), vectors [n x n_axes] (NaN columns from k on), status (_lib.PCOA_*), sweeps, rotations, k, n_negative, ms_kernel."""
    import numpy as np
    from ._lib import lib, check
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError("pcoa: dist must be a square matrix")
    n, n_axes = dist.shape[0], int(n_axes)
    eig, rel, pct = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
    vectors = np.zeros((max(n, 1), max(n_axes, 1)))
    info = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_pcoa(ctx._h, n, _dptr(dist), n_axes, _dptr(eig), _dptr(rel), _dptr(pct), _dptr(vectors), info, C.byref(ms)))
    return {"eig": eig, "rel_eig": rel, "axis_pct": pct, "vectors": vectors, "status": info[0], "sweeps": info[1], "rotations": info[2], "k": info[3],
            "n_negative": info[4], "ms_kernel": ms.value}


def pcoa_file(ctx, dist_path, directory, species=None):
    """The stage on files (msnv_pcoa_file): writes <species>_mann_pcoa_eig.tab and, unless fewer than two axes come out, <species>_mann_pcoa_proj.tab
    into directory.  Returns a dict: status (_lib.PCOA_*), sweeps, rotations, k, n_negative, n_samples, n_outliers, ms_kernel."""
    from ._lib import lib, check
    if species is None:
        species = os.path.basename(dist_path).split(".")[0]
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_pcoa_file(ctx._h, dist_path.encode(), directory.encode(), species.encode(), res, C.byref(ms)))
    return {"status": res[0], "sweeps": res[1], "rotations": res[2], "k": res[3], "n_negative": res[4], "n_samples": res[5], "n_outliers": res[6],
            "ms_kernel": ms.value}


def pcoa_subpops_main(argv=None):                              # clustering.R:120-126, :486-505 computePCoA
    import argparse
    ap = argparse.ArgumentParser(prog="pcoaSubpops.py", description="Ordinate a species' samples (subpopr's computePCoA: ape::pcoa of the distance matrix) on the GPU.")
    ap.add_argument("dist_file", metavar="DIST_FILE", help="<species>.filtered.mann.dist of metaSNV_DistDiv.py --dist")
    ap.add_argument("dir", metavar="DIR", help="holds the species' files of clusterSubpops.py: its output directory or the noClustering/ below it")
    ap.add_argument("--species", default=None, metavar="S", help="default: the dist file's name up to its first '.'")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    species = a.species if a.species is not None else os.path.basename(a.dist_file).split(".")[0]
    for f in (a.dist_file, os.path.join(a.dir, species + "_mann_clustering.tab")):
        if not os.path.exists(f):
            sys.exit("ERROR: missing input file: " + f)
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = pcoa_file(ctx, a.dist_file, a.dir, species=species)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    if res["status"] == core._lib.PCOA_TOO_FEW_AXES:
        print("Species " + species + ": Error during pcoa - check distance matrix (after optional filtering): " + str(res["k"]) + " axis")      # :125
    else:
        print("Species " + species + ": " + str(res["n_samples"]) + " samples ordinated, " + str(res["k"]) + " axes with a positive eigenvalue, "
              + str(res["n_negative"]) + " negative; " + str(res["sweeps"]) + " Jacobi sweeps")
    return res


def hclust_tasks(ctx, dist, tasks):
    """hclust of many index lists of dist [n x n], one workgroup per task (msnv_hclust_tasks).  tasks: (indices, method) pairs, method one of
    _lib.HCLUST_*.  Returns one dict per task: merge (int32 [m - 1, 2], R's hc$merge), height (float64 [m - 1]), order (0-based positions in the
    task's list, R's hc$order - 1); and the kernel's ms."""
    import numpy as np
    from ._lib import lib, check
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError("hclust_tasks: dist must be a square matrix")
    lists = [np.asarray(ix, dtype=np.int32).ravel() for ix, _ in tasks]
    m = np.array([len(x) for x in lists] + [0], dtype=np.int32)
    method = np.array([mt for _, mt in tasks] + [0], dtype=np.int32)
    idx = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, dtype=np.int32)]), dtype=np.int32)
    merge = np.zeros(2 * idx.size, dtype=np.int32)
    height = np.zeros(idx.size)
    order = np.zeros(idx.size, dtype=np.int32)
    ms = C.c_double()
    check(lib.msnv_hclust_tasks(ctx._h, dist.shape[0], _dptr(dist), len(tasks), _iptr(m), _iptr(method), _iptr(idx), _iptr(merge), _dptr(height), _iptr(order), C.byref(ms)))
    out, o = [], 0
    for t in range(len(tasks)):
        mt = int(m[t])
        out.append({"merge": merge[2 * (o - t):2 * (o - t + mt - 1)].reshape(mt - 1, 2).copy(), "height": height[o - t:o - t + mt - 1].copy(), "order": order[o:o + mt].copy()})
        o += mt
    return out, ms.value


def heatmap_order(merge, weights):
    """reorder(as.dendrogram(hc), weights), then order.dendrogram (msnv_heatmap_order; host only): the leaves left to right, 0-based, after the
    two children of every node are put in ascending order of their summed weights.  merge: hc$merge [m - 1, 2]."""
    import numpy as np
    from ._lib import lib, check
    merge = np.ascontiguousarray(merge, dtype=np.int32)
    weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
    m = weights.size
    if merge.size != 2 * max(m - 1, 0):
        raise ValueError("heatmap_order: merge must hold 2 (m - 1) entries for m weights")
    order = np.zeros(max(m, 1), dtype=np.int32)
    check(lib.msnv_heatmap_order(m, _iptr(merge), _dptr(weights), _iptr(order)))
    return order[:m]


def heatmap_file(ctx, dist_path, directory, species=None):
    """The stage on files (msnv_heatmap_file): writes <species>_mann_hclust_all.tab and _heatmap_all.tab and, when the directory holds a discovery
    subset of two samples or more, _hclust_discovery.tab and _heatmap_discovery.tab into directory.  Returns a dict: status (_lib.HEATMAP_*),
    n_samples, n_discovery, have_clustering, ms_kernel."""
    from ._lib import lib, check
    if species is None:
        species = os.path.basename(dist_path).split(".")[0]
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_heatmap_file(ctx._h, dist_path.encode(), directory.encode(), species.encode(), res, C.byref(ms)))
    return {"status": res[0], "n_samples": res[1], "n_discovery": res[2], "have_clustering": bool(res[3]), "ms_kernel": ms.value}


def heatmap_subpops_main(argv=None):                           # detailedSpeciesReport.rmd:142, :222, :250, :402
    import argparse
    ap = argparse.ArgumentParser(prog="heatmapSubpops.py", description="Order a species' samples for the report's distance heatmaps (hclust and the dendrogram reorder) on the GPU.")
    ap.add_argument("dist_file", metavar="DIST_FILE", help="<species>.filtered.mann.dist of metaSNV_DistDiv.py --dist")
    ap.add_argument("dir", metavar="DIR", help="holds the species' files of clusterSubpops.py: its output directory, or the noClustering/ or clustMedoidDefnFailed/ below it")
    ap.add_argument("--species", default=None, metavar="S", help="default: the dist file's name up to its first '.'")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    species = a.species if a.species is not None else os.path.basename(a.dist_file).split(".")[0]
    if not os.path.exists(a.dist_file):
        sys.exit("ERROR: missing input file: " + a.dist_file)
    if not os.path.isdir(a.dir):
        sys.exit("ERROR: missing directory: " + a.dir)
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = heatmap_file(ctx, a.dist_file, a.dir, species=species)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    print("Species " + species + ": " + str(res["n_samples"]) + " samples ordered (average linkage)"
          + ("; no discovery subset" if res["status"] == core._lib.HEATMAP_NO_DISCOVERY else "; " + str(res["n_discovery"]) + " of the discovery subset (complete linkage)"))
    return res


def freq_curves_geometry():
    """(rows, sample columns) that one block of msnv_freq_curves_k covers."""
    from ._lib import lib
    rows, cols = C.c_int32(), C.c_int32()
    lib.msnv_freq_curves_geometry(C.byref(rows), C.byref(cols))
    return rows.value, cols.value


def freq_curves(ctx, rows, strict_lo=10.0, strict_hi=90.0):
    """The cumulative counts behind snvFreqPlot of rows [n_pos x S] on the percent scale, NaN for no coverage (msnv_freq_curves).  Returns a dict:
    low [S, 50] (cells <= k), high [S, 50] (cells >= 100 - k), covered [S], strict [S] (cells < strict_lo or > strict_hi), all uint64, and ms_kernel."""
    import numpy as np
    from ._lib import lib, check
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2:
        raise ValueError("freq_curves: rows must be a positions x samples table")
    n_pos, S = rows.shape
    counts = np.zeros((max(S, 1), 102), dtype=np.uint64)
    ms = C.c_double()
    check(lib.msnv_freq_curves(ctx._h, _dptr(rows) if rows.size else None, n_pos, S, float(strict_lo), float(strict_hi), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                               C.byref(ms)))
    counts = counts[:S]
    return {"low": counts[:, :50].copy(), "high": counts[:, 50:100].copy(), "covered": counts[:, 100].copy(), "strict": counts[:, 101].copy(), "ms_kernel": ms.value}


def freq_bands(ctx, rows):
    """computeSnvFreqStats' three fixed bands of the same table (msnv_freq_bands): uint64 [S, 4] = cells outside 20/80, 10/90, 5/95 and covered
    cells; and the kernel's ms."""
    import numpy as np
    from ._lib import lib, check
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2:
        raise ValueError("freq_bands: rows must be a positions x samples table")
    n_pos, S = rows.shape
    counts = np.zeros((max(S, 1), 4), dtype=np.uint64)
    ms = C.c_double()
    check(lib.msnv_freq_bands(ctx._h, _dptr(rows) if rows.size else None, n_pos, S, counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ms)))
    return counts[:S], ms.value


def snv_freq_file(ctx, freq_path, out_dir, species=None, max_prop_reads_non_homog=0.1, min_prop_homog_snv=0.8, reserved=(0, 0)):
    """The stage on files (msnv_snvfreq_file): writes <species>_snvFreq_cutoffs.tab and <species>_snvFreq_fixed.tab into out_dir/snvFreqPlots/.
    Returns a dict: n_samples, n_rows, cutoff_index (0: no cutoff matches -x), n_used_for_medoid_defn (the plot's rule), n_selected (the
    clustering's rule), n_uncovered, ms_kernel."""
    from ._lib import lib, check, SnvFreqOpts
    if species is None:
        species = os.path.basename(freq_path).split(".")[0]
    opts = SnvFreqOpts()
    lib.msnv_snvfreq_opts_default(C.byref(opts))
    opts.max_prop_reads_non_homog, opts.min_prop_homog_snv = float(max_prop_reads_non_homog), float(min_prop_homog_snv)
    opts.reserved[0], opts.reserved[1] = int(reserved[0]), int(reserved[1])
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_snvfreq_file(ctx._h, freq_path.encode(), species.encode(), out_dir.encode(), C.byref(opts), res, C.byref(ms)))
    return {"n_samples": res[0], "n_rows": res[1], "cutoff_index": res[2], "n_used_for_medoid_defn": res[3], "n_selected": res[4], "n_uncovered": res[5],
            "ms_kernel": ms.value}


def snv_freq_subpops_main(argv=None):                          # snvFreqPlot.R:1-113; profileSubpops.R:152-158
    import argparse
    ap = argparse.ArgumentParser(prog="snvFreqSubpops.py", description="Write the numbers behind subpopr's SNV-frequency plots (snvFreqPlot) on the GPU.")
    ap.add_argument("freq_file", metavar="FREQ_FILE", help="<species>.filtered.freq of metaSNV_Filtering.py")
    ap.add_argument("out_dir", metavar="OUTDIR", help="the files go to OUTDIR/snvFreqPlots/")
    ap.add_argument("--species", default=None, metavar="S", help="default: the freq file's name up to its first '.'")
    ap.add_argument("--fix-read-threshold", type=float, default=0.1, metavar="X", help="subpopr -x: how far from 0 or 100 %% of reads an allele may be and count as fixed (0.1)")
    ap.add_argument("--fix-snv-threshold", type=float, default=0.8, metavar="Y", help="subpopr -y: the share of a sample's SNV positions that must be fixed (0.8)")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    species = a.species if a.species is not None else os.path.basename(a.freq_file).split(".")[0]
    if not os.path.exists(a.freq_file):
        sys.exit("ERROR: missing input file: " + a.freq_file)
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = snv_freq_file(ctx, a.freq_file, a.out_dir, species=species, max_prop_reads_non_homog=a.fix_read_threshold, min_prop_homog_snv=a.fix_snv_threshold)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    print("Species " + species + ": " + str(res["n_samples"]) + " samples, " + str(res["n_rows"]) + " rows; " + str(res["n_used_for_medoid_defn"]) + " pass the plot's rule ("
          + ("cutoffIndex " + str(res["cutoff_index"]) if res["cutoff_index"] else "no cutoffIndex matches " + repr(a.fix_read_threshold)) + "), "
          + str(res["n_selected"]) + " pass the selection rule")
    return res


def cluster_boot(ctx, dist, members, k, sets):
    """The PAM partition of dist's samples `members` (ascending indices) into k clusters, and how well each of its clusters is found again when
    every subset of `sets` (lists of distinct positions into members, clustered in the order given) is clustered on its own (msnv_cluster_boot).
    Returns cluster (1..k per member), medoids (positions in members), pairs [n_sets][k][2] = (inter, union) of every original cluster's best
    Jaccard match in every subset, and the kernels' ms."""
    import numpy as np
    from ._lib import lib, check
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError("cluster_boot: dist must be a square matrix")
    members = np.ascontiguousarray(members, dtype=np.int32).ravel()
    lists = [np.asarray(s, dtype=np.int32).ravel() for s in sets]
    set_m = np.array([len(s) for s in lists], dtype=np.int32)
    pos = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32), dtype=np.int32)
    k = int(k)
    med = np.zeros(max(k, 1), dtype=np.int32)
    clus = np.zeros(max(members.size, 1), dtype=np.int32)
    inter = np.zeros(max(len(lists) * max(k, 0), 1), dtype=np.int32)
    union = np.zeros_like(inter)
    ms = C.c_double()
    check(lib.msnv_cluster_boot(ctx._h, dist.shape[0], _dptr(dist), members.size, _iptr(members), k, len(lists), _iptr(set_m), _iptr(pos), _iptr(med), _iptr(clus),
                                _iptr(inter), _iptr(union), C.byref(ms)))
    nk = len(lists) * k
    pairs = np.stack([inter[:nk], union[:nk]], axis=1).reshape(len(lists), k, 2)
    return {"cluster": clus[:members.size].copy(), "medoids": med[:k].copy(), "pairs": pairs, "ms_kernel": ms.value}


STABILITY_SCORES = ("NA", "Low", "Medium", "High")


def membership_stability_file(ctx, dist_used_path, species, k, out_dir, clus_num_stability_path=None, seed=None, boot_iters=None):
    """The stage on files (msnv_membership_stability_file): writes <species>_mann_clusMembStability.tab and _stabilityAssessment.tab into out_dir.
    Returns a dict: status (_lib.MEMBSTAB_*), k, n_samples, n_proportions, n_sets, num_clusters_score and lowest_cluster_score (1 Low, 2 Medium,
    3 High, 0 NA), ms_kernel."""
    from ._lib import lib, check, MembStabOpts
    o = MembStabOpts()
    lib.msnv_membstab_opts_default(C.byref(o))
    if seed is not None:
        o.seed = int(seed)
    if boot_iters is not None:
        o.boot_iters = int(boot_iters)
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_membership_stability_file(ctx._h, dist_used_path.encode(), None if clus_num_stability_path is None else clus_num_stability_path.encode(),
                                             species.encode(), int(k), out_dir.encode(), C.byref(o), res, C.byref(ms)))
    return {"status": res[0], "k": res[1], "n_samples": res[2], "n_proportions": res[3], "n_sets": res[4], "num_clusters_score": res[5],
            "lowest_cluster_score": res[6], "ms_kernel": ms.value}


def _ps_values(path):
    """<species>_mann_PS_values.tab: a header "x", then k <TAB> mean prediction strength.  Returns {k: value}."""
    out = {}
    with open(path) as f:
        for ln in f.read().splitlines()[1:]:
            if ln:
                a, b = ln.split("\t")
                out[int(a)] = float(b)
    return out


def clusters_from_ps_values(directory, species, ps_cut=0.8):
    """The k msnv_cluster_file ran PAM with: the largest k whose prediction strength exceeds the cut; 1 when no PS values were written."""
    path = os.path.join(directory, species + "_mann_PS_values.tab")
    if not os.path.exists(path):
        return 1
    return max([k for k, v in _ps_values(path).items() if v > ps_cut] or [1])


def cluster_memb_stability_main(argv=None):                    # clustering.R:356-381 getClusteringResult, the membership half
    import argparse
    ap = argparse.ArgumentParser(prog="clusterMembStability.py", description="Rate how stable each subspecies cluster's membership is (subpopr's getClusMembStability) on the GPU.")
    ap.add_argument("species", metavar="SPECIES")
    ap.add_argument("dir", metavar="DIR", help="holds the species' files of clusterSubpops.py: its output directory or the noClustering/ below it")
    ap.add_argument("--k", type=int, default=None, metavar="N", help="number of clusters (default: from <species>_mann_PS_values.tab)")
    ap.add_argument("--ps-cut", type=float, default=0.8, metavar="X", help="prediction-strength cutoff used to pick k (0.8)")
    ap.add_argument("--seed", type=int, default=None, metavar="N")
    ap.add_argument("--boot", type=int, default=None, metavar="N", help="subsets per proportion (100)")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    dist_used = os.path.join(a.dir, a.species + "_mann_distMatrixUsedForClustMedoidDefns.txt")
    if not os.path.exists(dist_used):
        sys.exit("ERROR: missing input file: " + dist_used)
    k = a.k if a.k is not None else clusters_from_ps_values(a.dir, a.species, a.ps_cut)
    num_path = os.path.join(a.dir, a.species + "_mann_clusNumStability.tab")
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = membership_stability_file(ctx, dist_used, a.species, k, a.dir, clus_num_stability_path=num_path if os.path.exists(num_path) else None,
                                        seed=a.seed, boot_iters=a.boot)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    if res["status"] == core._lib.MEMBSTAB_NOT_RATED:
        print("Species " + a.species + ": " + str(res["n_samples"]) + " samples, fewer than 10: cluster stability is not rated")
    else:
        print("Species " + a.species + ": " + str(k) + " cluster(s), " + str(res["n_sets"]) + " subsets of " + str(res["n_samples"]) + " samples re-clustered; lowest cluster "
              "membership stability: " + STABILITY_SCORES[res["lowest_cluster_score"]])
    return res


def _csv_cell(v):
    """write.csv(quote = TRUE): strings quoted (a quote doubled), numbers and NA bare."""
    if v is None:
        return "NA"
    if isinstance(v, str):
        return '"' + v.replace('"', '""') + '"'
    if isinstance(v, float):
        return "%.15g" % v
    return str(v)


def _table(path):
    with open(path) as f:
        return [ln.split("\t") for ln in f.read().splitlines()[1:] if ln]


def summarise_clustering(out_dir):
    """summariseClusteringResultsForAll (src/subpopr/R/summariseClusteringResults.R:1-65) from the stage's files instead of the .rds: writes
    <out_dir>/summary_clustering.csv, one row per *_mann_clustering.tab of out_dir and out_dir/noClustering/.  Host only.  Returns the rows."""
    suffix = "_mann_clustering.tab"
    rels = [f for f in os.listdir(out_dir) if f.endswith(suffix)]
    none_dir = os.path.join(out_dir, "noClustering")
    if os.path.isdir(none_dir):
        rels += ["noClustering/" + f for f in os.listdir(none_dir) if f.endswith(suffix)]
    cols = ["speciesID", "speciesName", "numberOfSamplesUsedForClusterDetection", "numberOfClusters", "predictionStrengthValue", "confidenceInNumberOfClusters",
            "confidencePerCluster", "clusterSizes", "detailedClusteringResultsFile"]
    rows = []
    for rel in sorted(rels, key=lambda r: r.encode()):
        sub, name = os.path.split(rel)
        species = name[:-len(suffix)]
        prefix = os.path.join(out_dir, sub, species + "_mann")
        row = dict.fromkeys(cols)
        row["speciesID"] = species
        if os.path.exists(prefix + "_distMatrixUsedForClustMedoidDefns.txt"):
            row["numberOfSamplesUsedForClusterDetection"] = len(_table(prefix + "_distMatrixUsedForClustMedoidDefns.txt"))
        if os.path.exists(prefix + "_clusMembStability.tab"):
            memb = _table(prefix + "_clusMembStability.tab")
            first = [r for r in memb if r[2] == memb[0][2]]                 # the rows of the first proportion: one per cluster
            k = len(first)
            row["clusterSizes"] = "-".join(r[1] for r in first)
        else:
            k = clusters_from_ps_values(os.path.join(out_dir, sub), species)
        row["numberOfClusters"] = k
        if os.path.exists(prefix + "_PS_values.tab"):
            ps = _ps_values(prefix + "_PS_values.tab")
            if k in ps:
                row["predictionStrengthValue"] = float(round(ps[k], 4))
        if os.path.exists(prefix + "_stabilityAssessment.tab"):
            scores = dict(_table(prefix + "_stabilityAssessment.tab"))
            num = scores.get("numClusters", "NA")
            row["confidenceInNumberOfClusters"] = None if num == "NA" else num
            row["confidencePerCluster"] = "-".join(scores.get("clust%d" % (j + 1), "NA") for j in range(k))
        row["detailedClusteringResultsFile"] = "./" + (sub + "/" if sub else "") + species + "_detailedSpeciesReport.html"
        rows.append(row)
    text = ",".join(_csv_cell(c) for c in [""] + cols) + "\n"
    for row in rows:
        text += ",".join([_csv_cell(row["speciesID"])] + [_csv_cell(row[c]) for c in cols]) + "\n"
    with open(os.path.join(out_dir, "summary_clustering.csv"), "w") as f:
        f.write(text)
    return rows


def summarise_clustering_main(argv=None):                      # summariseClusteringResults.R:48-55 summariseClusteringResultsForAll
    import argparse
    ap = argparse.ArgumentParser(prog="summariseClustering.py", description="Write summary_clustering.csv for every species clustered into OUTDIR (subpopr's summariseClusteringResultsForAll).")
    ap.add_argument("out_dir", metavar="OUTDIR")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if not os.path.isdir(a.out_dir):
        sys.exit("ERROR: not a directory: " + a.out_dir)
    rows = summarise_clustering(a.out_dir)
    print(str(len(rows)) + " species summarised in " + os.path.join(a.out_dir, "summary_clustering.csv"))
    return rows


def genotype_rows(ctx, rows, clust, threshold=80.0):
    """computeUniquePosPerCluster's rule on arrays (msnv_genotype_rows).  rows [P x S] in 0..100 with NaN for no coverage; clust [S]: 0 for a
    column not in use, else 1..K.  Returns select and flip (uint32 [P], bit i - 1 = cluster i), n_rechecked (rows redone on the host in long
    double) and the kernel's ms."""
    import numpy as np
    from ._lib import lib, check
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    clust = np.ascontiguousarray(clust, dtype=np.int32).ravel()
    if rows.ndim != 2 or rows.shape[1] != clust.size:
        raise ValueError("genotype_rows: rows [P x S] and clust [S] must share S")
    p, s = rows.shape
    select, flip = np.zeros(max(p, 1), dtype=np.uint32), np.zeros(max(p, 1), dtype=np.uint32)
    n, ms = C.c_uint64(), C.c_double()
    u32 = C.POINTER(C.c_uint32)
    check(lib.msnv_genotype_rows(ctx._h, p, s, _dptr(rows), _iptr(clust), int(clust.max(initial=0)), float(threshold), select.ctypes.data_as(u32),
                                 flip.ctypes.data_as(u32), C.byref(n), C.byref(ms)))
    return {"select": select[:p], "flip": flip[:p], "n_rechecked": n.value, "ms_kernel": ms.value}


def genotype_file(ctx, clustering_path, freq_path, out_dir, species=None, uniq_threshold=0.8):
    """The stage on files (msnv_genotype_file).  Returns a dict: status (_lib.GENOTYPE_*), n_clusters, n_samples, n_rows, n_positions,
    n_rechecked, n_correct, n_good, ms_kernel."""
    from ._lib import lib, check
    if species is None:
        species = os.path.basename(freq_path).split(".")[0]
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_genotype_file(ctx._h, clustering_path.encode(), freq_path.encode(), species.encode(), out_dir.encode(), float(uniq_threshold), res, C.byref(ms)))
    return {"status": res[0], "n_clusters": res[1], "n_samples": res[2], "n_rows": res[3], "n_positions": res[4], "n_rechecked": res[5], "n_correct": res[6],
            "n_good": res[7], "ms_kernel": ms.value}


GENOTYPE_ENDINGS = {                                           # what <species>_hap_out.txt ends with (writeGenotypeFreqs.R:12-105)
    1: "a single cluster: nothing to genotype",
    2: "no genotyping positions",
    3: "at least one cluster is missing genotyping positions",
    4: "the genotype-specific SNV frequency cutoff is bad",
}


def write_genotype_freqs_main(argv=None):                      # writeGenotypeFreqs.R:2-112
    import argparse
    ap = argparse.ArgumentParser(prog="writeGenotypeFreqs.py", description="Select each subspecies' genotyping SNVs (subpopr's writeGenotypeFreqs) on the GPU.")
    ap.add_argument("species", metavar="SPECIES")
    ap.add_argument("clustering", metavar="CLUSTERING_TAB", help="<species>_mann_clustering.tab of clusterSubpops.py")
    ap.add_argument("freq", metavar="FREQ_FILE", help="<species>.filtered.freq")
    ap.add_argument("out_dir", metavar="OUTDIR")
    ap.add_argument("--uniq-threshold", type=float, default=0.8, metavar="X", help="mean frequency difference to every other cluster, as a proportion (0.8)")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    for f in (a.clustering, a.freq):
        if not os.path.exists(f):
            sys.exit("ERROR: missing input file: " + f)
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = genotype_file(ctx, a.clustering, a.freq, a.out_dir, species=a.species, uniq_threshold=a.uniq_threshold)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    if res["status"] in GENOTYPE_ENDINGS:
        print("Species " + a.species + ": " + GENOTYPE_ENDINGS[res["status"]] + " (see " + os.path.join(a.out_dir, a.species + "_hap_out.txt") + ")")
    else:
        print("Species " + a.species + ": " + str(res["n_positions"]) + " genotyping positions for " + str(res["n_clusters"]) + " clusters from " + str(res["n_rows"])
              + " SNVs; " + str(res["n_correct"]) + " of " + str(res["n_good"]) + " classified samples assigned to their own cluster")
    return res


def profile_columns(ctx, rows, flip, cols_per_pass=0):
    """Per column of rows [G x S] (0..100, NaN for no coverage; a row with flip[g] set counts as 100 - x): the counts and the two middle order
    statistics of its called cells (msnv_subpop_profile_columns).  Returns n_called, n_gt0, n_ge5, n_eq0, n_eq100 (uint32 [S]), mid_lo, mid_hi
    (float64 [S]: ranks (n - 1) // 2 and n // 2, NaN at n = 0) and the kernel's ms.  cols_per_pass: the width of a column band (0: from free memory)."""
    import numpy as np
    from ._lib import lib, check
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    flip = np.ascontiguousarray(flip).astype(np.uint8).ravel()
    if rows.ndim != 2 or rows.shape[0] != flip.size:
        raise ValueError("profile_columns: rows [G x S] and flip [G] must share G")
    g, s = rows.shape
    out = {k: np.zeros(max(s, 1), dtype=np.uint32) for k in ("n_called", "n_gt0", "n_ge5", "n_eq0", "n_eq100")}
    lo, hi = np.zeros(max(s, 1)), np.zeros(max(s, 1))
    ms = C.c_double()
    u32 = C.POINTER(C.c_uint32)
    check(lib.msnv_subpop_profile_columns(ctx._h, g, s, _dptr(rows), flip.ctypes.data_as(C.POINTER(C.c_uint8)), int(cols_per_pass),
                                          *[out[k].ctypes.data_as(u32) for k in ("n_called", "n_gt0", "n_ge5", "n_eq0", "n_eq100")], _dptr(lo), _dptr(hi), C.byref(ms)))
    res = {k: v[:s] for k, v in out.items()}
    res.update(mid_lo=lo[:s], mid_hi=hi[:s], ms_kernel=ms.value)
    return res


def subpop_profile_files(ctx, species, out_dir, all_samples_path, max_prop_uncalled=0.2, min_genotype_abundance=80.0):
    """writeSubpopsForAllSamples on files (msnv_subpop_profile_files).  Returns a dict: status (_lib.PROFILE_*), n_files, n_usable, n_full, n_filtered,
    n_incoherent, n_bad, n_assigned, ms_kernel."""
    from ._lib import lib, check
    res = (C.c_int64 * 8)()
    ms = C.c_double()
    check(lib.msnv_subpop_profile_files(ctx._h, species.encode(), out_dir.encode(), all_samples_path.encode(), float(max_prop_uncalled), float(min_genotype_abundance),
                                        res, C.byref(ms)))
    return {"status": res[0], "n_files": res[1], "n_usable": res[2], "n_full": res[3], "n_filtered": res[4], "n_incoherent": res[5], "n_bad": res[6],
            "n_assigned": res[7], "ms_kernel": ms.value}


def subpop_abundance_files(species, out_dir, abundance_path, sample_suffix=None):
    """writeSubpopAbundSpeciesAbund on files (msnv_subpop_abundance_files; host only).  Returns (samples used, clusters, samples in wFreq.tab,
    sample columns of the abundance table)."""
    from ._lib import lib, check
    counts = (C.c_uint64 * 4)()
    check(lib.msnv_subpop_abundance_files(species.encode(), out_dir.encode(), abundance_path.encode(), None if sample_suffix is None else sample_suffix.encode(), counts))
    return tuple(counts)


PROFILE_ENDINGS = {                                            # what <species>_extended_clustering_stat.txt ends with (writeSubpopsForAllSamples.R:16-117)
    1: "no <species>_*.pos.freq file: run getGenotypingSNVSubset.py and convertSNVtoAlleleFreq.py first",
    2: "no cluster had usable placing data",
}


def profile_subpops_main(argv=None):                           # profileSubpops.R:228-274 useGenotypesToProfileSubpops
    import argparse
    ap = argparse.ArgumentParser(prog="profileSubpops.py", description="Profile subspecies in every sample (subpopr's useGenotypesToProfileSubpops) on the GPU.")
    ap.add_argument("species", metavar="SPECIES")
    ap.add_argument("metasnv_dir", metavar="METASNV_DIR", help="metaSNV's output directory (holds all_samples)")
    ap.add_argument("out_dir", metavar="OUTDIR", help="holds <species>_<cluster>.pos.freq and <species>_<cluster>_hap_positions.tab")
    ap.add_argument("--max-prop-uncalled", type=float, default=0.2, metavar="X", help="a sample is kept when it has at least X * (genotyping positions) called (0.2)")
    ap.add_argument("--min-genotype-abundance", type=float, default=80.0, metavar="X", help="median above which a sample is assigned to a cluster (80)")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    median_path = os.path.join(a.out_dir, a.species + "_hap_freq_median.tab")
    if not os.path.exists(median_path):                        # :243-248
        print("No distinctive genotyping positions for species " + a.species + ", perhaps the cutoff was bad. See "
              + os.path.join(a.out_dir, a.species + "_hap_out.txt") + " for details. (Required file does not exist: " + median_path + ")")
        return None
    all_samples = os.path.join(a.metasnv_dir, "all_samples")
    if not os.path.exists(all_samples):                        # :250-254
        sys.exit("ERROR: File with paths to samples does not exist. This should have been created by metaSNV.Expected path: " + all_samples)
    from . import core
    try:
        ctx = core.Context(0)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    try:
        res = subpop_profile_files(ctx, a.species, a.out_dir, all_samples, a.max_prop_uncalled, a.min_genotype_abundance)
    except core._lib.MsnvError as e:
        sys.exit("ERROR: {}".format(e))
    finally:
        ctx.close()
    if res["status"] in PROFILE_ENDINGS:
        print("Species " + a.species + ": " + PROFILE_ENDINGS[res["status"]])
        print("Species does not have cluster frequencies. Species: " + a.species)      # :269-271
    else:
        print("Species " + a.species + ": " + str(res["n_usable"]) + " of " + str(res["n_files"]) + " clusters profiled; " + str(res["n_filtered"]) + " of "
              + str(res["n_full"]) + " samples kept, " + str(res["n_assigned"]) + " assigned to a cluster")
        if res["n_filtered"] == 0:
            print("Species does not have cluster frequencies. Species: " + a.species)
    return res


def write_subpop_abund_main(argv=None):                        # profileSubpops.R:277-310 useSpeciesAbundToCalcSubspeciesAbund, species abundances
    import argparse
    ap = argparse.ArgumentParser(prog="writeSubpopAbund.py", description="Scale subspecies frequencies by the species' abundance (subpopr's writeSubpopAbundSpeciesAbund).")
    ap.add_argument("species", metavar="SPECIES")
    ap.add_argument("out_dir", metavar="OUTDIR", help="holds <species>_extended_clustering_wFreq.tab")
    ap.add_argument("abundance", metavar="SPECIES_ABUNDANCE_FILE", help="species x samples table: first line the sample names, first column the species")
    ap.add_argument("--sample-suffix", default=None, metavar="S", help="appended to the table's sample names when none matches")
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    freq_path = os.path.join(a.out_dir, a.species + "_extended_clustering_wFreq.tab")
    if not os.path.exists(freq_path):                          # :280-283
        print("Species " + a.species + " does not have cluster frequencies. File does not exist: " + freq_path)
        return None
    if not os.path.exists(a.abundance):                        # :291-296
        sys.exit("ERROR: Cannot compute overall subspecies abundances. Required species abundance file not found: " + a.abundance)
    from ._lib import MsnvError
    try:
        return subpop_abundance_files(a.species, a.out_dir, a.abundance, a.sample_suffix)
    except MsnvError as e:
        sys.exit("ERROR: {}".format(e))
