"""subpopr's two raw-SNV consumers, same argv and the same files as the reference scripts:

  getGenotypingSNVSubset.py <hapDir> <metaSNVdir>     (src/subpopr/inst/getGenotypingSNVSubset.py)
      <hapDir>/*hap_positions.tab + <metaSNVdir>/snpCaller/called_SNPs*  ->  <hapDir>/<species>.pos
  convertSNVtoAlleleFreq.py <file.pos> <minDepth>     (src/subpopr/inst/convertSNVtoAlleleFreq.py)
      <file.pos>  ->  <file.pos>.freq

  correlateSubpopProfileWithGeneProfiles.py <species> <outDir> <geneAbundanceFile> <geneFamilyType> [--sample-suffix S]
      (src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R, the function's argument order)
      <outDir>/<species>_allClust_relativeAbund.tab + the gene-family table  ->  <outDir>/<species>_corr<type>-{spearman,pearson,
      clusterSpecificGenes,speciesSpecificGenes}.tsv

The first is a text filter (native, no device work); the frequencies of the second and the correlations of the third are
computed on the GPU (msnv_snv_allele_freq, msnv_gene_corr, msnv_corr_stats) and there is no CPU fallback for them."""
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
