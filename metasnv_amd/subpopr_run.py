"""subpopr end to end, the reference's fourth command line (metaSNV_subpopr.R:65-784 with defineSubpopulations, src/subpopr/R/profileSubpops.R:38-213):

  metaSNV_subpopr.py -i METASNV_DIR [-o results] [-p N] [-s SUFFIX] [-a SPECIES_ABUNDANCE -m FALSE] [-g GENE_ABUNDANCE] [-r TRUE] [--minNumSamples 100]
                     [-x 0.1] [-y 0.8] [-z 0.8] [--clusterPSThreshold 0.8] [-q FALSE] [--useExistingClustering FALSE] [--useExistingGenotyping FALSE]
                     [--seed N] [--device N] [--stability-iters N] [--boot N]

One process and one core.Context run every stage of metasnv_amd/subpopr.py for every species of the project: the species' front door (NA cells out
of the distance table, the samples both tables hold, the size checks), snvFreqPlot's numbers, the clustering with -x / -y, its two stability ratings
and the PCoA, the genotyping SNVs; then, over the project, the raw-SNV subset, the allele frequencies, the subspecies profiles, their abundances and
the gene-content correlations, and the reference's summaries.  A species that fails is recorded with its message and the run goes on (the
reference's bptry); a failed HIP call ends the run at once.  Everything that computes is a stage's kernel; there is no CPU fallback.  What is on the
host here: argument handling, the NA rule (integers), and the summaries (small tables).  Divergences: DESIGN.md section 7."""
import glob
import os
import re
import sys
import time

from . import subpopr

NA_CELLS = ("NA", "")


def r_number(v):
    """A double as R pastes it into a path or a table: 15 significant digits."""
    return "%.15g" % v


def _logical(text):
    """optparse's type = "logical" (metaSNV_subpopr.R:96-168)."""
    import argparse
    if text in ("TRUE", "T", "true"):
        return True
    if text in ("FALSE", "F", "false"):
        return False
    raise argparse.ArgumentTypeError("a logical is TRUE, FALSE, T, F, true or false, not '%s'" % text)


def parse_args(argv):
    import argparse
    ap = argparse.ArgumentParser(prog="metaSNV_subpopr.py", description="Detect and profile subspecies in every species of a metaSNV project (subpopr) on the GPU.")
    ap.add_argument("-i", "--metaSnvResultsDir", default=None, metavar="DIR", help="metaSNV's output directory (required)")
    ap.add_argument("-o", "--outputDir", default="results", metavar="DIR")
    ap.add_argument("-p", "--procs", type=int, default=1, metavar="N", help="accepted and ignored: one process drives the device")
    ap.add_argument("-s", "--sampleSuffix", default="", metavar="S", help="the constant suffix behind the sample names in metaSNV's bam files")
    ap.add_argument("-a", "--speciesAbundance", default="doNotRun", metavar="FILE", help="species x samples abundance table")
    ap.add_argument("-m", "--isMotus", type=_logical, default=True, metavar="LOGICAL", help="the abundance table is a mOTUs2 profile (TRUE; that variant is not built)")
    ap.add_argument("-g", "--geneAbundance", default="doNotRun", metavar="FILE", help="gene family x samples abundance table")
    ap.add_argument("-r", "--createReports", type=_logical, default=True, metavar="LOGICAL", help="write the numbers behind the reports' heatmaps (no HTML is written)")
    ap.add_argument("--minNumSamples", type=float, default=100, metavar="N")
    ap.add_argument("-x", "--fixReadThreshold", type=float, default=0.1, metavar="X")
    ap.add_argument("-y", "--fixSnvThreshold", type=float, default=0.8, metavar="Y")
    ap.add_argument("-z", "--genotypingThreshold", type=float, default=0.8, metavar="Z")
    ap.add_argument("--clusterPSThreshold", type=float, default=0.8, metavar="PS")
    ap.add_argument("-q", "--onlyDoSubspeciesDetection", type=_logical, default=False, metavar="LOGICAL")
    ap.add_argument("--useExistingClustering", type=_logical, default=False, metavar="LOGICAL")
    ap.add_argument("--useExistingGenotyping", type=_logical, default=False, metavar="LOGICAL")
    ap.add_argument("--seed", type=int, default=None, metavar="N", help="seed of every draw (the stages' default: 1)")
    ap.add_argument("--device", type=int, default=0, metavar="N")
    ap.add_argument("--stability-iters", type=int, default=None, metavar="N", help="subsamples per proportion of the cluster-number stability (10)")
    ap.add_argument("--boot", type=int, default=None, metavar="N", help="subsets per proportion of the membership stability (100)")
    a = ap.parse_args(argv)
    if a.metaSnvResultsDir is None:                            # metaSNV_subpopr.R:212-215
        ap.print_help()
        sys.exit("Path to metaSNV results must be supplied [-i]")
    for name in ("fixReadThreshold", "fixSnvThreshold", "genotypingThreshold", "clusterPSThreshold"):      # assert0to1, :225-234
        v = getattr(a, name)
        if not (0.0 <= v <= 1.0):
            sys.exit("Param \"" + name + "\"must be numeric and must be between 0 and 1")
    for path, kind in ((a.speciesAbundance, "Species abundance"), (a.geneAbundance, "Gene family abundance"), (a.metaSnvResultsDir, "MetaSNV output directory")):   # checkFile, :238-251
        if path and path != "doNotRun" and not os.path.exists(path):
            sys.exit(kind + " file specified but does not exist: " + path)
    if a.speciesAbundance != "doNotRun" and a.isMotus:
        sys.exit("ERROR: -a " + a.speciesAbundance + " with -m TRUE: the mOTU variant of the abundance stage (writeSubpopAbundMotusProfile) is not built. "
                 "Pass -m FALSE with a species x samples abundance table.")
    return a


def out_dir_of(a):
    """OUT.DIR (metaSNV_subpopr.R:256-261)."""
    params = "params.hr" + r_number(a.fixReadThreshold * 100) + ".hs" + r_number(a.fixSnvThreshold * 100) + ".ps" + r_number(a.clusterPSThreshold * 100) \
        + ".gs" + r_number(a.genotypingThreshold * 100)
    return os.path.join(a.outputDir, params, os.path.basename(os.path.normpath(a.metaSnvResultsDir)))


class Log:
    """What the run prints goes to the screen and to OUT/log.txt."""

    def __init__(self, path):
        self.f = open(path, "w")

    def say(self, msg=""):
        print(msg)
        self.f.write(msg + "\n")
        self.f.flush()

    def warn(self, msg):
        self.say("Warning: " + msg)

    def close(self):
        self.f.close()


# ---------------------------------------------------------------------------------------------- the species' front door
def species_of(metasnv_dir):
    """(species in both places, species in one only), each in byte order (metaSNV_subpopr.R:331-348)."""
    def names(sub, tail):
        d = os.path.join(metasnv_dir, sub)
        found = set()
        for f in (os.listdir(d) if os.path.isdir(d) else []):
            sp = f.split(".")[0]
            if f == sp + tail:
                found.add(sp)
        return found
    dist, freq = names("distances", ".filtered.mann.dist"), names(os.path.join("filtered", "pop"), ".filtered.freq")
    order = lambda s: sorted(s, key=lambda x: x.encode())
    return order(dist & freq), order(dist ^ freq)


def read_dist_text(path):
    """<species>.filtered.mann.dist as text: (names, cells[n][n]).  The cells stay as written, so a cleaned copy holds the survivors' text unchanged."""
    with open(path) as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    lines = [ln for i, ln in enumerate(lines) if i == 0 or ln]
    if not lines:
        raise ValueError(path + ": empty file")
    names = lines[0].split("\t")[1:]
    cells = []
    for i, ln in enumerate(lines[1:]):
        f = ln.split("\t")
        if len(f) != len(names) + 1 or i >= len(names) or f[0] != names[i]:
            raise ValueError("%s:%d: a row of %d cells that follows the header's order is expected" % (path, i + 2, len(names)))
        cells.append(f[1:])
    if len(cells) != len(names):
        raise ValueError("%s: %d rows for %d samples" % (path, len(cells), len(names)))
    return names, cells


def rm_na_from_dist_matrix(cells):
    """rmNAfromDistMatrix (rmNAsfromDistMatrix.R): the indices of the samples that stay, ascending.  Samples whose row or column is all NA go; then the
    sample with the most NA cells in its column goes, the first in matrix order on ties, until no NA is left.  The counts are kept up to date per
    removal: O(n^2) in all."""
    n = len(cells)
    na = [[c in NA_CELLS for c in row] for row in cells]
    row_all = [all(na[i]) for i in range(n)]
    col_all = [all(na[i][j] for i in range(n)) for j in range(n)]
    alive = [not (row_all[i] or col_all[i]) for i in range(n)]
    col = [sum(1 for i in range(n) if alive[i] and na[i][j]) if alive[j] else 0 for j in range(n)]      # NA cells of column j among the rows that stay
    total = sum(col)
    while total > 0:
        worst = -1
        for j in range(n):
            if alive[j] and (worst < 0 or col[j] > col[worst]):
                worst = j
        alive[worst] = False
        total -= col[worst]                                    # its column
        col[worst] = 0
        for j in range(n):                                     # its row
            if alive[j] and na[worst][j]:
                col[j] -= 1
                total -= 1
    return [i for i in range(n) if alive[i]]


def write_dist_text(path, names, cells, keep):
    with open(path, "w") as f:
        f.write("\t" + "\t".join(names[i] for i in keep) + "\n")
        for i in keep:
            f.write(names[i] + "\t" + "\t".join(cells[i][j] for j in keep) + "\n")


def freq_header(path):
    with open(path) as f:
        return f.readline().rstrip("\r\n").split("\t")[1:]


def clean_inputs(sp, dist_path, freq_path, out_dir, min_samples, log):
    """Steps 1-4 of the front door (profileSubpops.R:74-141).  Returns (dist path for the stages, None) or (None, the reference's reason)."""
    names, cells = read_dist_text(dist_path)
    keep = rm_na_from_dist_matrix(cells)
    fnames = freq_header(freq_path)
    n_freq = len(fnames)
    if [names[i] for i in keep] != fnames:                     # :86-99
        in_freq = set(fnames)
        keep = [i for i in keep if names[i] in in_freq]
        n_freq = len(keep)
        log.warn("Samples names do not match in the distance matrix and the filtered SNV file for species " + sp + ". Using the intersection, which is "
                 + str(len(keep)) + " samples.")
        if len(keep) < min_samples:
            log.warn("Too few samples remain after selecting only those in the distance and SNP files. At least " + r_number(min_samples)
                     + " are required for analysis. Aborting for species: " + sp)
            return None, "Too few samples remain after selecting only those in the distance and SNP files. At least " + r_number(min_samples) + " are required for analysis."
    if n_freq < min_samples:                                   # :133-136
        log.warn("Insufficient number of samples in metaSNV filtered SNV results for species: " + sp + " (" + str(len(keep)) + " samples)")
        return None, "Insufficient number of samples in metaSNV filtered SNV results (" + str(len(keep)) + " samples)"
    if len(keep) < 2 or len(keep) < min_samples:               # :138-141
        log.warn("Insufficient number of samples in metaSNV dist matrix results for species: " + sp + " (" + str(len(keep)) + " samples)")
        return None, "Insufficient number of samples in metaSNV dist matrix results (" + str(len(keep)) + " samples)"
    if len(keep) == len(names):
        return dist_path, None
    inputs = os.path.join(out_dir, "inputs")
    os.makedirs(inputs, exist_ok=True)
    cleaned = os.path.join(inputs, sp + ".filtered.mann.dist")
    write_dist_text(cleaned, names, cells, keep)
    log.say("Species " + sp + ": " + str(len(names) - len(keep)) + " of " + str(len(names)) + " samples left out of the distance table; the stages read " + cleaned)
    return cleaned, None


def _n_clusters_in(path):
    return len({r[1] for r in subpopr._table(path)})


def define_subpopulations(ctx, sp, a, out_dir, log, ms):
    """defineSubpopulations for one species: its result string.  ms: a one-entry list the stages' kernel milliseconds are added to."""
    from . import _lib
    dist_path = os.path.join(a.metaSnvResultsDir, "distances", sp + ".filtered.mann.dist")
    freq_path = os.path.join(a.metaSnvResultsDir, "filtered", "pop", sp + ".filtered.freq")
    log.say("Checking data for species: " + sp)
    dist_path, reason = clean_inputs(sp, dist_path, freq_path, out_dir, a.minNumSamples, log)
    if reason is not None:
        return reason
    log.say("Plotting SNV frequencies for species: " + sp)
    ms[0] += subpopr.snv_freq_file(ctx, freq_path, out_dir, species=sp, max_prop_reads_non_homog=a.fixReadThreshold, min_prop_homog_snv=a.fixSnvThreshold)["ms_kernel"]
    none_dir = os.path.join(out_dir, "noClustering")
    existing = [p for p in (os.path.join(out_dir, sp + "_mann_clustering.tab"), os.path.join(none_dir, sp + "_mann_clustering.tab")) if os.path.exists(p)]
    if a.useExistingClustering and existing:                   # :162-178
        log.say("Using existing clustering for species: " + sp + " (" + existing[0] + ")")
        clustering_path = existing[0]
        k = _n_clusters_in(clustering_path)
    else:
        log.say("Computing clustering for species: " + sp)
        res = subpopr.cluster_file(ctx, dist_path, out_dir, species=sp, freq_path=freq_path, seed=a.seed, ps_cut=a.clusterPSThreshold, stability_iters=a.stability_iters,
                                   max_prop_reads_non_homog=a.fixReadThreshold, min_prop_homog_snv=a.fixSnvThreshold)
        ms[0] += res["ms_kernel"]
        status = res["status"]
        if status in (_lib.CLUSTER_OK, _lib.CLUSTER_NONE):
            d = out_dir if status == _lib.CLUSTER_OK else none_dir
            num_path = os.path.join(d, sp + "_mann_clusNumStability.tab")
            st = subpopr.membership_stability_file(ctx, os.path.join(d, sp + "_mann_distMatrixUsedForClustMedoidDefns.txt"), sp,
                                                   subpopr.clusters_from_ps_values(d, sp, a.clusterPSThreshold), d,
                                                   clus_num_stability_path=num_path if os.path.exists(num_path) else None, seed=a.seed, boot_iters=a.boot)
            ms[0] += st["ms_kernel"]
            pc = subpopr.pcoa_file(ctx, dist_path, d, species=sp)
            ms[0] += pc["ms_kernel"]
            if pc["status"] == _lib.PCOA_TOO_FEW_AXES:
                return "Error during pcoa - check distance matrix (after optional filtering): " + sp       # clustering.R:125
        if status in subpopr.CLUSTER_REASONS:
            return subpopr.CLUSTER_REASONS[status] + (" (n samples = " + str(res["n_samples"]) + ")" if status == _lib.CLUSTER_TOO_FEW else "")
        k = res["n_clusters"]
        clustering_path = os.path.join(out_dir if status == _lib.CLUSTER_OK else none_dir, sp + "_mann_clustering.tab")
    if k <= 1:
        log.say("No significant clustering detected for species: " + sp)
        return "nClusters = 1"
    log.say("Identifying distinctive SNVs for clusters in species: " + sp)
    ms[0] += subpopr.genotype_file(ctx, clustering_path, freq_path, out_dir, species=sp, uniq_threshold=a.genotypingThreshold)["ms_kernel"]
    return "nClusters = " + str(k)


class DeviceFailure(Exception):
    """A HIP call failed: nothing more is launched."""


def run_species(ctx, species, a, out_dir, log, ms):
    from . import _lib
    results = {}
    for sp in species:
        log.say("")
        log.say("=== Assessing presence of subspecies in species " + sp + " ===")
        try:
            results[sp] = define_subpopulations(ctx, sp, a, out_dir, log, ms)
        except _lib.MsnvError as e:
            if e.code == _lib.EHIP:
                raise DeviceFailure("species " + sp + ": " + str(e))
            results[sp] = "ERROR: " + str(e)
        except (OSError, ValueError) as e:
            results[sp] = "ERROR: " + str(e)
        log.say("Species " + sp + ": " + results[sp])
    return results


def guarded(log, what, fn, *args, **kw):
    """One stage call of the project-wide part: a failure other than a HIP error is printed and the run goes on.  Returns the stage's result or None."""
    from . import _lib
    try:
        return fn(*args, **kw)
    except _lib.MsnvError as e:
        if e.code == _lib.EHIP:
            raise DeviceFailure(what + ": " + str(e))
        log.say("ERROR: " + what + ": " + str(e))
        return None


# ---------------------------------------------------------------------------------------------- the summaries (host only)
def _bytes_order(names):
    return sorted(names, key=lambda x: x.encode())


def _quoted(s):
    return '"' + s.replace('"', '""') + '"'


def write_results_per_species(out_dir, results):
    """write.table(stack(results), row.names = F) (metaSNV_subpopr.R:424-429)."""
    esc = lambda s: '"' + s.replace('"', '\\"') + '"'
    with open(os.path.join(out_dir, "log_clusteringSummaryPerSpecies.txt"), "w") as f:
        f.write('"result" "species"\n')
        for sp, res in results.items():
            f.write(esc(res) + " " + esc(sp) + "\n")


def clustered_species(out_dir):
    """The species summary_clustering.csv has a row for: a *_mann_clustering.tab in out_dir or out_dir/noClustering/."""
    suffix = "_mann_clustering.tab"
    found = set()
    for d in (out_dir, os.path.join(out_dir, "noClustering")):
        if os.path.isdir(d):
            found.update(f[:-len(suffix)] for f in os.listdir(d) if f.endswith(suffix))
    return _bytes_order(found)


def _line_count(path):
    with open(path) as f:
        return len(f.read().splitlines())


def summarise_clustering_extension(out_dir):
    """summariseClusteringExtensionResultsForAll (summariseClusteringResults.R:70-127): writes summary_clusteringExtension.csv, returns its rows."""
    rows = []
    listing = _bytes_order(os.listdir(out_dir))
    for sp in clustered_species(out_dir):
        init = os.path.join(out_dir, "noClustering", sp + "_mann_clustering.tab")
        ext = os.path.join(out_dir, sp + "_extended_clustering.tab")
        if os.path.exists(init) and _n_clusters_in(init) == 1:
            rows.append((sp, "No clusters", "NA", "NA"))
        elif os.path.exists(ext):
            sizes = {}
            for r in subpopr._table(ext):
                if r[1] != "NA":
                    sizes[int(r[1])] = sizes.get(int(r[1]), 0) + 1
            pattern = re.compile(sp + "_.*_hap_positions.tab")             # getSnvGenotypingCount: the species id as a regex, not anchored
            n_snvs = [_line_count(os.path.join(out_dir, f)) - 1 for f in listing if pattern.search(f)]
            rows.append((sp, "Succeeded", "-".join(str(sizes[c]) for c in sorted(sizes)), "-".join(map(str, n_snvs))))
        else:
            rows.append((sp, "Failed", "NA", "NA"))
    with open(os.path.join(out_dir, "summary_clusteringExtension.csv"), "w") as f:
        f.write('"speciesID","ClusterGenotyping","GenotypedClusterSizes","nSNVs"\n')
        for r in rows:
            f.write(",".join(_quoted(c) for c in r) + "\n")
    return rows


def _r_sum(values):
    """R's sum(): one pass in long double."""
    import numpy as np
    s = np.longdouble(0)
    for v in values:
        s += np.longdouble(v)
    return float(s)


def assess_subpop_completeness(out_dir):
    """assessSubpopCompleteness (assessSubpopCompleteness.R:8-53) over every <species>_extended_clustering_wFreq.tab: writes subpopFreqSumsStats.tsv
    (without the taxonomy columns), returns its rows; nothing is written without such a file."""
    suffix = "_extended_clustering_wFreq.tab"
    stats = []
    for f in _bytes_order(x for x in os.listdir(out_dir) if x.endswith(suffix)):
        with open(os.path.join(out_dir, f)) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln]
        n_clus = len(lines[0].split("\t")) if lines else 0
        sums = [_r_sum(float("nan") if c in ("NA", "NaN") else float(c) for c in ln.split("\t")[1:]) for ln in lines[1:]]
        n = len(sums)
        if n == 0:
            continue
        # length(freqSum[cond]): an NA in cond selects an NA, which length() counts
        prop = lambda cond: sum(1 for s in sums if s != s or cond(s)) / n
        row = [f[:-len(suffix)], n_clus, n, prop(lambda s: s == 100), prop(lambda s: s > 100), prop(lambda s: s > 110), prop(lambda s: s > 120),
               prop(lambda s: s < 100), prop(lambda s: s < 90), prop(lambda s: s < 80), prop(lambda s: s < 50)]
        eq100, gt100, gt120, lt90, lt50 = row[3], row[4], row[6], row[8], row[10]
        row.append(eq100 < 0.8 or gt100 > 0.05 or lt90 > 0.05 or gt120 != 0 or lt50 != 0)
        stats.append(row)
    if not stats:
        return stats
    stats.sort(key=lambda r: (not r[11], r[3]))                # arrange(desc(warningFlag), eq100); sort() is stable
    with open(os.path.join(out_dir, "subpopFreqSumsStats.tsv"), "w") as f:
        f.write("species\tnClus\tnSamples\teq100\tgt100\tgt110\tgt120\tlt100\tlt90\tlt80\tlt50\twarningFlag\n")
        for r in stats:
            f.write("\t".join([r[0], str(r[1]), str(r[2])] + [r_number(v) for v in r[3:11]] + ["TRUE" if r[11] else "FALSE"]) + "\n")
    return stats


def collect_subpop_abunds(out_dir):
    """collectSubpopAbunds (collectSubpopAbunds.R): writes subpopAbunds.tsv from every *hap_coverage_extended_normed.tab, the abundance cells as read.
    Returns the number of rows, None without such a file."""
    files = _bytes_order(f for f in os.listdir(out_dir) if re.search(".*hap_coverage_extended_normed.tab", f))
    if not files:
        return None
    rows = []
    for f in files:
        parts = f.split("_")
        for r in subpopr._table(os.path.join(out_dir, f)):
            rows.append((r[0], parts[0], parts[2], r[1]))
    rows.sort(key=lambda r: r[0].encode())
    with open(os.path.join(out_dir, "subpopAbunds.tsv"), "w") as fh:
        fh.write("sampleName\tspecies\tsubpop\tabundance\n")
        for r in rows:
            fh.write("\t".join(r) + "\n")
    return len(rows)


def _has_rows(path):
    """fileExistsAndHasRows (summariseClusteringResults.R:207-213)."""
    return os.path.exists(path) and _line_count(path) > 1


def summarise_gene_family_correlations(out_dir, family_type):
    """summariseGeneFamilyCorrelationResultsForAll (summariseClusteringResults.R:177-225): writes summary_geneFamilyCorrAssoc.csv, returns its rows."""
    rows = []
    for sp in clustered_species(out_dir):
        prefix = os.path.join(out_dir, sp + "_corr" + family_type)
        res = [p for p in (prefix + "-spearman.tsv", prefix + "-pearson.tsv") if os.path.exists(p)]
        if not res:
            worked, report = "No correlation results", None
        else:
            worked = ("Correlation results empty", "Only one correlation result file present", "Correlations calculated")[sum(_has_rows(p) for p in res)]
            report = "./" + sp + "_geneContentReport.html"
        rows.append((sp, worked, _has_rows(prefix + "-clusterSpecificGenes.tsv"), report))
    with open(os.path.join(out_dir, "summary_geneFamilyCorrAssoc.csv"), "w") as f:
        f.write('"speciesID","geneFamCorrTested","anySignifGeneFamCorrs","detailedGeneFamCorrResultsFile"\n')
        for sp, worked, sig, report in rows:
            f.write(",".join([_quoted(sp), _quoted(worked), "TRUE" if sig else "FALSE", "NA" if report is None else _quoted(report)]) + "\n")
    return rows


def _csv_cells(line):
    """The cells of one line of write.csv(quote = T), each as written (quotes kept)."""
    cells, cur, quoted = [], "", False
    for ch in line:
        if ch == '"':
            quoted = not quoted
        if ch == "," and not quoted:
            cells.append(cur)
            cur = ""
        else:
            cur += ch
    cells.append(cur)
    return cells


def _read_csv(path, drop_first):
    with open(path) as f:
        rows = [_csv_cells(ln) for ln in f.read().splitlines() if ln]
    return [r[1:] for r in rows] if drop_first else rows


def combine_all_summaries(out_dir):
    """combineAllSummaries (summariseClusteringResults.R:227-250) from the .csv files instead of the .rds: summary_clustering.csv without its row
    names, merged by speciesID with the extension and gene-family summaries that exist; every cell stays as written."""
    full = _read_csv(os.path.join(out_dir, "summary_clustering.csv"), True)
    for name in ("summary_clusteringExtension.csv", "summary_geneFamilyCorrAssoc.csv"):
        path = os.path.join(out_dir, name)
        if not os.path.exists(path):
            continue
        other = _read_csv(path, False)
        by_id = {}
        for r in other[1:]:
            by_id.setdefault(r[0], r[1:])
        full = [full[0] + other[0][1:]] + [r + by_id[r[0]] for r in full[1:] if r[0] in by_id]
    full[1:] = sorted(full[1:], key=lambda r: r[0].encode())
    with open(os.path.join(out_dir, "summary_allResults.csv"), "w") as f:
        for r in full:
            f.write(",".join(r) + "\n")
    return len(full) - 1


# ---------------------------------------------------------------------------------------------- the driver
def _stage_dist_path(a, out_dir, sp):
    cleaned = os.path.join(out_dir, "inputs", sp + ".filtered.mann.dist")
    return cleaned if os.path.exists(cleaned) else os.path.join(a.metaSnvResultsDir, "distances", sp + ".filtered.mann.dist")


def run(ctx, a, out_dir, log, summary, ms):
    species, left_out = species_of(a.metaSnvResultsDir)
    log.say("Using files from " + a.metaSnvResultsDir + "/distances and " + a.metaSnvResultsDir + "/filtered/pop/")
    if left_out:
        log.warn("Species indicated in " + a.metaSnvResultsDir + "/distances and " + a.metaSnvResultsDir + "/filtered/pop/ are not identical. Using the intersection ("
                 + str(len(species)) + " species). Species not found in both locations: " + ",".join(left_out))
    if not species:
        log.say("No appropriate files found in " + a.metaSnvResultsDir)
        sys.exit("No appropriate files found in " + a.metaSnvResultsDir)
    summary["species"] = {}
    log.say("Running subpopr on " + str(len(species)) + " species in one process.")

    if not a.useExistingClustering:                            # metaSNV_subpopr.R:416-500
        results = run_species(ctx, species, a, out_dir, log, ms)
        summary["species"] = results
        write_results_per_species(out_dir, results)
        log.say("Summarising clustering results.")
        subpopr.summarise_clustering(out_dir)
    else:                                                      # :501-520
        log.say("Using previously computed clustering.")
        if a.useExistingGenotyping:
            log.say("Using previously computed genotyping SNVs.")
        else:
            log.say("Identifying genotyping SNVs...")
            summary["species"] = run_species(ctx, species, a, out_dir, log, ms)
        if not os.path.exists(os.path.join(out_dir, "summary_clustering.csv")):
            sys.exit("ERROR: --useExistingClustering TRUE, but " + os.path.join(out_dir, "summary_clustering.csv") + " of an earlier run does not exist")
    tail = "_hap_out.txt"
    with_substructure = _bytes_order(f[:-len(tail)] for f in os.listdir(out_dir) if f.endswith(tail))
    log.say("Species with substructure: " + str(len(with_substructure)) + "/" + str(len(species)))

    if a.onlyDoSubspeciesDetection and not a.useExistingClustering:       # :443-446
        combine_all_summaries(out_dir)
        log.say("Subpopr stopped due to 'onlyDoSubspeciesDetection' flag being true")
        return

    if a.createReports:                                        # the numbers behind the three kinds of detailed report; no HTML
        dirs = [out_dir] if a.useExistingClustering else [out_dir, os.path.join(out_dir, "noClustering"), os.path.join(out_dir, "clustMedoidDefnFailed")]
        suffix = "_mann_clustering.tab"
        for d in dirs:
            for sp in (_bytes_order(f[:-len(suffix)] for f in os.listdir(d) if f.endswith(suffix)) if os.path.isdir(d) else []):
                res = guarded(log, "heatmap order of species " + sp, subpopr.heatmap_file, ctx, _stage_dist_path(a, out_dir, sp), d, species=sp)
                if res is not None:
                    ms[0] += res["ms_kernel"]

    if not with_substructure:                                  # :528-532
        log.say("Substructure not detected in any species (" + str(len(species)) + " tested). Aborting.")
        summarise_clustering_extension(out_dir)
        combine_all_summaries(out_dir)
        return

    log.say("Gather genotyping SNV frequencies")               # :543-578
    if a.useExistingGenotyping:
        log.say("Using previously gathered genotyping SNV frequencies (.pos and .pos.freq files)")
    else:
        log.say("Gathering genotyping SNV profiles")
        haps = sorted(glob.glob(os.path.join(out_dir, "*hap_positions.tab")), key=lambda x: x.encode())
        snps = sorted(glob.glob(os.path.join(a.metaSnvResultsDir, "snpCaller", "called_SNPs*")), key=lambda x: x.encode())
        if not haps or not snps:
            log.say("ERROR:  no " + ("*hap_positions.tab files" if not haps else "/snpCaller/called_SNPs* files in metaSNV output directory"))
            log.say("Skipping subspecies genotyping.")
        else:
            guarded(log, "genotyping SNV subset", subpopr.genotyping_subset, haps, snps, out_dir)
        all_pos = _bytes_order(f for f in os.listdir(out_dir) if re.search(r".*_.*\.pos$", f))
        if not all_pos:
            log.warn("Genotyping failed. No *.pos files found. Not genotyping subspecies.")
        else:
            log.say("Calculating genotyping SNVs frequencies")
            for f in all_pos:
                res = guarded(log, "allele frequencies of " + f, subpopr.snv_allele_freq, ctx, os.path.join(out_dir, f), 5)
                if res is not None:
                    ms[0] += res[1]

    log.say("Determining abundance of clusters using genotyping SNVs")      # :580-593
    all_samples = os.path.join(a.metaSnvResultsDir, "all_samples")
    for sp in with_substructure:
        median_path = os.path.join(out_dir, sp + "_hap_freq_median.tab")
        if not os.path.exists(median_path):
            log.warn("No distinctive genotyping positions for species " + sp + ", perhaps the cutoff was bad. See " + os.path.join(out_dir, sp + "_hap_out.txt")
                     + " for details. (Required file does not exist: " + median_path + ")")
        elif not os.path.exists(all_samples):
            log.say("ERROR: File with paths to samples does not exist. This should have been created by metaSNV.Expected path: " + all_samples)
        else:
            res = guarded(log, "subspecies profiles of species " + sp, subpopr.subpop_profile_files, ctx, sp, out_dir, all_samples)
            if res is not None:
                ms[0] += res["ms_kernel"]
                if res["status"] != 0 or res["n_filtered"] == 0:
                    log.warn("Species does not have cluster frequencies. Species: " + sp)
    summarise_clustering_extension(out_dir)
    assess_subpop_completeness(out_dir)                        # :628-633

    have_abundance = a.speciesAbundance != "doNotRun"
    if have_abundance:                                         # :637-665
        log.say("Calculating cluster abundances using species abundances...")
        for sp in with_substructure:
            freq_path = os.path.join(out_dir, sp + "_extended_clustering_wFreq.tab")
            if not os.path.exists(freq_path):
                log.warn("Species " + sp + " does not have cluster frequencies. File does not exist: " + freq_path)
            else:
                guarded(log, "subspecies abundances of species " + sp, subpopr.subpop_abundance_files, sp, out_dir, a.speciesAbundance, a.sampleSuffix or None)
        if collect_subpop_abunds(out_dir) is None:
            log.warn("Subspecies abundance calculations failed. No expected results files exist (.*hap_coverage_extended_normed.tab). See log files.")

    if a.geneAbundance != "doNotRun" and have_abundance:       # :708-769
        log.say("Testing for gene correlations for " + str(len(with_substructure)) + " species")
        log.say("Correlating cluster and gene family abundances (Pearson & Spearman)...")
        for sp in with_substructure:
            clust_path = os.path.join(out_dir, sp + "_allClust_relativeAbund.tab")
            if not os.path.exists(clust_path):
                log.say("No cluster abundances file for species " + sp + ". May be due to failed genotyping. Missing required file for gene content calculation: " + clust_path)
            else:
                guarded(log, "gene correlations of species " + sp, subpopr.gene_corr_files, ctx, clust_path, a.geneAbundance, os.path.join(out_dir, sp + "_corrGenes"),
                        a.sampleSuffix or None)
        summarise_gene_family_correlations(out_dir, "Genes")
    elif a.geneAbundance != "doNotRun":
        log.say("Not running gene content analysis. Species abundances (-a) are required for it.")

    log.say("Summarising results...")                          # :772-783
    combine_all_summaries(out_dir)
    log.say("Results summarised, see: " + os.path.join(out_dir, "summary_allResults.csv"))
    log.say("Subpopr finished.")


def main(argv=None):
    """Returns the run's summary(): species (name -> result string), out_dir, wall_s, ms_kernel."""
    argv = list(sys.argv[1:] if argv is None else argv)
    a = parse_args(argv)
    from . import core
    t0 = time.time()
    try:
        ctx = core.Context(a.device)
    except core._lib.MsnvError as e:
        sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU (there is no CPU fallback)\n".format(e))
    out_dir = out_dir_of(a)
    summary = {"species": {}, "out_dir": out_dir, "wall_s": 0.0, "ms_kernel": 0.0}
    ms = [0.0]
    log = None
    try:
        os.makedirs(out_dir, exist_ok=True)
        log = Log(os.path.join(out_dir, "log.txt"))
        log.say("Command was --------------------------------------------------")
        log.say("metaSNV_subpopr.py " + " ".join(argv))
        log.say("Variable values --------------------------------------------------")
        for k in sorted(vars(a)):
            log.say(k + " : " + str(getattr(a, k)))
        log.say("OUT.DIR : " + out_dir)
        log.say("Run output --------------------------------------------------")
        run(ctx, a, out_dir, log, summary, ms)
    except DeviceFailure as e:
        if log:
            log.say("ERROR: a HIP call failed; nothing more is launched. " + str(e))
        sys.exit("ERROR: a HIP call failed; nothing more is launched. " + str(e))
    finally:
        summary["wall_s"] = time.time() - t0
        summary["ms_kernel"] = ms[0]
        if log:
            log.say("wall seconds: %.3f; kernel milliseconds: %.3f" % (summary["wall_s"], summary["ms_kernel"]))
            log.close()
        ctx.close()
    return summary
