/*
 * include/msnv.h -- C ABI of libmsnv.so, the MI355X-native pileup SNV caller.
 *
 * The reference (metaSNV) has no plugin API on this path: its hot path is two PROCESS
 * boundaries driven by metaSNV.py.  Each entry point below names the process invocation
 * (argv + files + exit status) it replaces, so a maintainer can swap the subprocess call
 * for one ctypes call (the stub is shown in INTEGRATION.md).
 *
 *   msnv_coverage()  <-  `qaCompute -c 10 -d -i BAM OUT`            metaSNV.py:55-78
 *                        (src/qaTools/qaCompute.cpp:286-681)
 *   msnv_call()      <-  `samtools mpileup -f REF [-l SPLIT] -B -b LIST |
 *                         snpCall -f REF [-g ANN] -i INDIV -c C -t T > CALLED`
 *                                                                    metaSNV.py:153-176
 *                        (src/snpCaller/call_vC.cpp:330-679)
 *
 * The staged msnv_dataset_* / msnv_pileup_run / msnv_write_calls entry points are the same
 * path cut at its natural seams (decode+pack | device kernels | text), so that a caller
 * can keep the packed columns resident in HBM (bench.py times msnv_pileup_run only).
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on
 * success and a positive MSNV_E* code otherwise (the reference's drivers treat any
 * non-zero exit status as fatal: metaSNV.py:75-78,212-221); the message is available from
 * msnv_last_error() (thread-local) and echoed to stderr.  The library never abort()s.
 * All compute runs on the GPU: there is no CPU fallback, and every entry point fails with
 * MSNV_ENODEV when no HIP device is usable.
 */
#ifndef MSNV_H
#define MSNV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSNV_OK        0
#define MSNV_EINVAL    1   /* bad argument                                              */
#define MSNV_EIO       2   /* cannot open / read / write a file                         */
#define MSNV_EFORMAT   3   /* malformed BAM / FASTA / BED / annotation                  */
#define MSNV_ENODEV    4   /* no usable HIP device (the path never falls back to CPU)   */
#define MSNV_EHIP      5   /* a HIP runtime call or kernel launch failed                */
#define MSNV_ENOMEM    6
#define MSNV_EDOMAIN   7   /* input outside the domain of the reference tools (SURVEY.md
                              Appendix A "D" items), e.g. BAM without mapped reads       */
#define MSNV_ECAPACITY 8   /* internal device buffer too small (caller may retry)        */

typedef struct msnv_ctx     msnv_ctx;      /* one per GPU / per rank          */
typedef struct msnv_dataset msnv_dataset;  /* packed read columns of one shard */

int         msnv_abi_version(void);
const char *msnv_last_error(void);

/* Number of visible HIP devices (hipGetDeviceCount; 0 when the runtime has none). */
int  msnv_device_count(void);
int  msnv_ctx_create(int device_id, msnv_ctx **out);
void msnv_ctx_destroy(msnv_ctx *ctx);

/* ------------------------------------------------------------------------------------
 * Calling parameters = snpCall's options (call_vC.cpp:26-36,382-390) + the mpileup
 * defaults metaSNV relies on (metaSNV.py:160-165 passes none).
 * ------------------------------------------------------------------------------------ */
typedef struct {
    int32_t min_coverage;        /* snpCall -c, default 4                                 */
    int32_t calling_threshold;   /* snpCall -t, default 4                                 */
    double  min_fraction;        /* snpCall -p, default 0.01 (never passed by metaSNV.py) */
    int32_t min_baseq;           /* mpileup -Q, default 13                                */
    int32_t flag_filter;         /* mpileup --ff, default 0x704                           */
    int32_t count_orphans;       /* mpileup -A, default 0                                 */
    int32_t max_depth;           /* mpileup -d, default 8000 (per file)                   */
    int32_t min_mapq;            /* mpileup -q, default 0                                 */
    int32_t drop_first_line;     /* 1 = reproduce call_vC.cpp:423 (first pileup position of
                                    the invocation is consumed for sample counting and never
                                    called); 0 = call every position                      */
    int32_t cov_max;             /* qaCompute -c, default 10                              */
    int32_t cov_min_mapq;        /* qaCompute -q, default 1                               */
    int32_t ignore_overlaps;     /* mpileup -x, default 0: the overlapping-mate quality tweak is ON, as in the
                                    reference's command line (metaSNV.py:160-165 passes no -x)             */
    int32_t token_limit;         /* snpCall's per-token character limit (call_vC.cpp:482: 10000): a sample's
                                    base string is cut there, bases behind the cut are not counted; 0 = unlimited */
} msnv_params;

void msnv_params_default(msnv_params *p);

/* ------------------------------------------------------------------------------------
 * msnv_coverage  <-  qaCompute -c <max_cov> -d -i <bam_path> <out_cov_path>
 * Writes <out_cov_path> and <out_detail_path> byte-for-byte as qaCompute.cpp:192-217,
 * 226-263,439,623-657 would.  Return: 0 ok (qaCompute.cpp:680); MSNV_EIO mirrors its
 * exit 1 (:53-57,376-379); MSNV_EDOMAIN for the inputs on which it has undefined
 * behaviour (no mapped reads: :596).
 * ------------------------------------------------------------------------------------ */
typedef struct {
    const char *bam_path;
    int32_t     max_cov;          /* -c, metaSNV passes 10 */
    int32_t     min_mapq;         /* -q, default 1         */
    const char *out_cov_path;     /* OUT                   */
    const char *out_detail_path;  /* OUT.detail (-d)       */
} msnv_cov_args;

int msnv_coverage(msnv_ctx *ctx, const msnv_cov_args *args);

/* ------------------------------------------------------------------------------------
 * msnv_call  <-  samtools mpileup -f ref_fasta [-l bed_split_path] -B -b <bam list> |
 *                snpCall -f ref_fasta [-g ann_path] -i out_indiv_path -c .. -t .. [-p ..]
 *                > out_called_path
 * Sample order = bam_paths order = all_samples order (call_vC.cpp:530).
 * contig_rank_mask: optional (NULL = all): one byte per BAM-header contig, non-zero =
 * this rank's shard (multi-GPU contig sharding); output then holds
 * only those contigs.
 * ------------------------------------------------------------------------------------ */
typedef struct {
    const char *const *bam_paths;
    int32_t     n_bams;
    const char *ref_fasta;        /* -f                                                  */
    const char *ann_path;         /* -g or NULL                                          */
    const char *bed_split_path;   /* -l or NULL: 3-column `name\t1\tLEN` (metaSNV.py:92)  */
    const char *out_called_path;  /* stdout of snpCall                                   */
    const char *out_indiv_path;   /* -i or NULL                                          */
    const uint8_t *contig_rank_mask;
    int32_t     n_contig_rank_mask;
    int32_t     host_threads;     /* BAM decode threads, 0 = auto                        */
    msnv_params params;
} msnv_call_args;

int msnv_call(msnv_ctx *ctx, const msnv_call_args *args);

/* msnv_call_from_mpileup  <-  snpCall -f ref_fasta [-g ann_path] -i out_indiv_path -c -t [-p] < mpileup.txt > out_called_path
 * (call_vC.cpp:346-410 options, :423-668 main loop): snpCall on its own input, the TEXT `samtools mpileup -f REF -B -b LIST`
 * writes -- the reference's literal process boundary, for pipelines that already hold pileup text and for
 * A/B runs against real samtools output.  The text is parsed and called on the device (csrc/textcall.hip): first line = sample
 * count, never processed (:423-431); toksplit's 10 000-character tokens (:92-111); ^x / +n / -n / * $ N n (:503-535); gates and
 * calling rule (:545-601); gene / codon annotation with both ann_path and ref_fasta (:448).
 *   text / text_bytes: the pileup text in memory; or text = NULL and mpileup_path names a file ("-" or NULL: stdin).
 *   out_indiv_path may be NULL (individual SNVs are then dropped, :653-660).  Of params only min_coverage, calling_threshold and
 *   min_fraction apply (the mpileup options were spent by whoever wrote the text).
 *   stats (may be NULL): [0] lines read, [1] samples, [2] called_SNPs lines, [3] indiv_called lines, [4] kernel microseconds,
 *   [5] text bytes parsed on the device, [6] base-string characters parsed, [7] the most lines
 *   one wavefront of the parser handled in a launch (ceil(lines / wavefronts), the largest over the chunks of the text).
 * Input the reference crashes on (a pileup symbol outside its ten keys, e.g. '>' '<' from CIGAR N or an IUPAC letter; more samples
 * in a line than in the first) is MSNV_EDOMAIN and nothing is written. */
typedef struct {
    const char *text; uint64_t text_bytes;
    const char *mpileup_path;
    const char *ref_fasta;        /* may be NULL without ann_path */
    const char *ann_path;         /* may be NULL                  */
    const char *out_called_path;
    const char *out_indiv_path;   /* may be NULL                  */
    msnv_params params;
} msnv_mpileup_args;
int msnv_call_from_mpileup(msnv_ctx *ctx, const msnv_mpileup_args *args, uint64_t stats[8]);

/* ------------------------------------------------------------------------------------
 * Next row of the path: metaSNV_Filtering.py filter_two
 * (metaSNV_Filtering.py:156-242) -- position filter and allele frequencies of the called
 * positions, computed on the device for all species of interest in one pass over the files.
 * ------------------------------------------------------------------------------------ */
typedef struct {
    const char        *species;     /* TaxID = contig name up to the first '.' (:172)              */
    int32_t            n_soi;       /* samples of interest of this species (relevant_taxa, :111-145) */
    const int32_t     *soi;         /* their indices in all_samples order (:180-181)                */
    const char *const *soi_names;   /* header of <species>.filtered.freq (:203)                     */
} msnv_filter_species;

/* snp_paths: the snpCaller/called* (or indiv*) files, in the order they are to be read.  Writes
 * out_dir/<species>.filtered.freq for every species with at least one surviving position (-c min_cov_c,
 * -p min_prop_p; defaults 5.0 and 0.50).  n_positions_kept / ms_kernel may be NULL. */
/* repr() of a Python float, the text metaSNV_Filtering.py:231 prints for a frequency (shortest digits that
 * round-trip; exponent form below 1e-4 and from 1e16).  Returns the length, or -1 when cap is too small. */
int msnv_format_float(double x, char *buf, int32_t cap);

int msnv_filter_files(msnv_ctx *ctx, const char *const *snp_paths, int32_t n_paths, int32_t n_samples,
                      const msnv_filter_species *species, int32_t n_species, double min_cov_c, double min_prop_p,
                      const char *out_dir, uint64_t *n_positions_kept, double *ms_kernel);
/* The same filter fed from the records of the dataset's last msnv_pileup_run instead of the text of called_SNPs /
 * indiv_called (no S-wide lines are written, read back and split): which = 0 the population calls (what called_SNPs
 * holds), 1 the individual calls (indiv_called, metaSNV_Filtering.py --ind).  ann_path / fasta_path as for msnv_write_calls
 * (gene column and codon tags of the row ids), or NULL.  Writes the same bytes as msnv_filter_files on the written files. */
struct msnv_dataset;
int msnv_filter_resident(struct msnv_dataset *ds, int32_t which, const msnv_filter_species *species, int32_t n_species,
                         double min_cov_c, double min_prop_p, const char *out_dir, const char *ann_path, const char *fasta_path,
                         uint64_t *n_positions_kept, double *ms_kernel);

/* metaSNV_DistDiv.py --dist (computeDist, metaSNV_DistDiv.py:105-124): pairwise sample
 * distances of one species' *.filtered.freq table on the device, bit-exact with pandas (NaN-skipping mean whose sum is
 * numpy's pairwise summation).  Writes the manhattan (mean |f1 - f2|) and the allele (share of positions with
 * |f1 - f2| > threshold, 0.6 in the reference) matrices as DataFrame.to_csv(sep='\t') does.  Out pointers may be NULL. */
/* The value pandas' default CSV float converter (precise_xstrtod) gives `text` -- what computeDist sees after
 * pd.read_table; not always the correctly rounded one.  Returns 0, or MSNV_EFORMAT when text is not a plain number or
 * overflows a double (beyond 1e308, where pandas leaves the column as text). */
int msnv_parse_float(const char *text, double *value);

int msnv_dist_file(msnv_ctx *ctx, const char *freq_path, const char *mann_path, const char *allele_path, double threshold,
                   int32_t *n_samples, uint64_t *n_positions, double *ms_kernel);

/* metaSNV_DistDiv.py --div / --divNS (computeDiv / computeDivNS, metaSNV_DistDiv.py:144-301): pairwise nucleotide
 * diversity of one species' *.filtered.freq table on the device, bit-exact with pandas / numpy (compute_diversity for
 * every pair of samples: single rows and multi-allelic positions, numpy's pairwise summation in 8192-element blocks,
 * pandas' Kahan groupby sum), divided by the coverage corrections on the host.
 *   mode MSNV_DIV:    out_a = <species>.diversity, out_b = <species>.FST
 *   mode MSNV_DIV_NS: out_a = <species>.N_diversity, out_b = <species>.S_diversity (MSNV_EDOMAIN when the table has
 *                     no N row or no S row, where the reference raises)
 *   matched:          keep only the positions filt_proportion keeps (the reference's --matched)
 *   genome_length:    sum of bed_header's column 3 over the species' contigs (L)
 *   horizontal / vertical: the species' Percentage_1x / Average_cov per sample of the table's header, n_samples_cov of each
 *   row_order:        the permutation sort_index applies to the rows' contig:gene:pos keys (numpy's argsort of them,
 *                     quicksort for MSNV_DIV, stable for MSNV_DIV_NS; identity when already sorted); must sort the keys
 * Writes the lower-triangular matrices as DataFrame.to_csv(sep='\t') does.  Out pointers may be NULL; ms_kernel is the
 * kernels' time summed over the tables.  A position key with more than 55 rows (after the class split and the matched
 * filter) is MSNV_EDOMAIN before any launch, with ms_kernel 0 and neither file written: its m(m-1)+1 values per sample
 * make an outer product one lane would sum for more than a second per pair. */
#define MSNV_DIV    0
#define MSNV_DIV_NS 1
int msnv_div_file(msnv_ctx *ctx, const char *freq_path, int32_t mode, int32_t matched, int64_t genome_length,
                  const double *horizontal, const double *vertical, int32_t n_samples_cov, const int64_t *row_order,
                  uint64_t n_rows_order, const char *out_a, const char *out_b, int32_t *n_samples, uint64_t *n_rows,
                  double *ms_kernel);

/* subpopr's raw-SNV consumers.
 *
 * msnv_genotyping_subset -- src/subpopr/inst/getGenotypingSNVSubset.py:20-48: the positions listed in every
 * <species>_hap_positions.tab (field 2 = contig:gene:pos:base), then one scan of the called_SNPs* files that copies each
 * line whose contig:pos is wanted into out_dir/<species>.pos of every species that listed it.  The path lists are read
 * in the order given (the reference walks glob.glob's directory order).  Text only: runs without a device.
 *
 * msnv_snv_allele_freq -- src/subpopr/inst/convertSNVtoAlleleFreq.py:7-24: writes <pos_path>.freq, one row per allele
 * of every line: id contig:gene:pos:base, then per sample -1 (coverage below min_depth) or count / coverage * 100,
 * computed on the device and printed like str(float).  Every line of one file must list the same number of samples. */
int msnv_genotyping_subset(const char *const *hap_paths, int32_t n_hap, const char *const *snp_paths, int32_t n_snp,
                           const char *out_dir, uint64_t *n_positions, uint64_t *n_lines_written);
int msnv_snv_allele_freq(msnv_ctx *ctx, const char *pos_path, int32_t min_depth, uint64_t *n_rows, double *ms_kernel);

/* subpopr's correlateSubpopProfileWithGeneProfiles (src/subpopr/R/correlateSubpopProfileWithGeneProfiles.R): every cluster's
 * abundance vector against every gene family's, Spearman and Pearson, on the device in fp64.
 *
 * msnv_gene_corr -- the array form (doCorr, :141-153).  clust holds n_clusters rows of n_samples values (the caller appends the
 * species row, the column sums), genes n_genes rows; both row-major, already cut to the samples and genes in use.  For
 * every (cluster c, gene g), at [c * n_genes + g]: rho = Pearson coefficient of the average ranks, r = Pearson coefficient of
 * log10(v + pseudocount), valid = 0 where either raw vector has max == min (rho and r are then NaN).  *pseudocount = the smallest
 * cell above 0 of genes / 1000.  3 <= n_samples <= 8192 (one workgroup ranks a row in LDS), else MSNV_EDOMAIN; negative or
 * non-finite cells, or no cell above 0, are MSNV_EDOMAIN too.  pseudocount / ms_kernel may be NULL.
 *
 * msnv_corr_stats -- cor.test's derived columns of one table and p.adjust(p, "BH") over its n rows: per row the statistic
 * (MSNV_CORR_PEARSON: sqrt(n_obs - 2) e / sqrt(1 - e^2); MSNV_CORR_SPEARMAN: (n_obs^3 - n_obs)(1 - e) / 6), the two-sided p of
 * the t approximation (exact = FALSE), for Pearson the Fisher interval (NaN at n_obs = 3; conf_low / conf_high may be NULL)
 * and q.  An estimate of exactly +-1 gives p = 0 and, for Pearson, an infinite statistic.  n_obs < 3 is MSNV_EDOMAIN.
 *
 * msnv_gene_corr_files -- the whole stage: reads <species>_allClust_relativeAbund.tab (write.table's layout) and the gene-family
 * table (TSV, '#' lines skipped, header id + samples), keeps the clusters seen in >= 3 samples, the samples both tables hold
 * (retrying with gene column + sample_suffix when none match and a suffix is given; none at all: MSNV_EDOMAIN) and the genes
 * present in them, and writes <out_prefix>-spearman.tsv, -pearson.tsv, -clusterSpecificGenes.tsv and -speciesSpecificGenes.tsv
 * (selectSubspeciesSpecificGenes with its defaults, :238-303).  counts = clusters tested, genes kept, samples used, specific
 * genes; all 0 and nothing written when no cluster is seen in 3 samples.  A cell that is NA, empty or not a number is
 * MSNV_EFORMAT (R drops such pairs silently). */
#define MSNV_CORR_PEARSON  0
#define MSNV_CORR_SPEARMAN 1
int msnv_gene_corr(msnv_ctx *ctx, int32_t n_clusters, int64_t n_genes, int32_t n_samples, const double *clust, const double *genes,
                   double *rho, double *r, uint8_t *valid, double *pseudocount, double *ms_kernel);
int msnv_corr_stats(msnv_ctx *ctx, int32_t method, uint64_t n, const double *estimate, const int32_t *n_obs, double *statistic,
                    double *p_value, double *conf_low, double *conf_high, double *q_value);
int msnv_gene_corr_files(msnv_ctx *ctx, const char *clust_abund_path, const char *gene_abund_path, const char *sample_suffix,
                         const char *out_prefix, uint64_t counts[4]);

/* subpopr's computeClusters -> getClusteringResult (src/subpopr/R/clustering.R:20-133, :289-427): how many subspecies a species has and
 * which samples belong to which.  Every PAM run is one workgroup of one launch; the n x n distance matrix (row-major fp64, 2 <= n <=
 * 4096) stays on the device.  It must be symmetric with a zero diagonal (pam sees a dist object), every cell finite and >= 0: anything
 * else is MSNV_EDOMAIN.
 *
 * msnv_pam_tasks -- cluster::pam(diss = TRUE, pamonce = 0) of many index subsets.  Task t is task_m[t] sample indices (its list, in idx
 * behind the lists of the tasks before it) and task_k[t], 1 <= k < m.  Out, in the same packing: medoids (task_k[t] positions in the
 * task's list, 0-based, ascending; packed behind each other), cluster (per list entry, 1..k, numbered by ascending medoid position) and
 * n_swaps[t].  The rules, restated from pam.c (unpinned, no R was run):
 *   BUILD   dysma[j] = 1.1 max(d) + 1 (max over the task's sub-matrix); k times: beter[i] = sum over j ascending of (dysma[j] - d(i,j)
 *           where that is > 0) for every non-medoid i, the LAST i with the largest beter becomes a medoid, dysma[j] = min(dysma[j],
 *           d(i,j)); sky = sum of dysma[j], j ascending
 *   SWAP    (k > 1) dysma[j] / dysmb[j] = nearest / second nearest medoid distance, medoids ascending, strict <; for every non-medoid h
 *           ascending and medoid i ascending, dz = sum over j ascending of: d(i,j) == dysma[j] ? min(dysmb[j], d(h,j)) - dysma[j] :
 *           d(h,j) < dysma[j] ? d(h,j) - dysma[j] : nothing; the FIRST smallest dz < 1 is dzsky; swapped while dzsky < -16 DBL_EPSILON
 *           |sky|, sky += dzsky
 *   assign  nearest medoid, medoids ascending, strict <
 * All sums are sequential fp64 sums without contraction, so the result is a function of the task alone, not of its place in the batch.
 *
 * msnv_pred_strength -- predStrengthCustom (:152-216) for given permutations: perms holds, for k = 2..k_max and l = 0..M-1 in that
 * order, one permutation of 0..n-1 (n entries each).  Its first floor(n / 2) entries are half 1, the rest half 2; both are clustered
 * by PAM, every member is classified by the OTHER half's medoids (nearest, first on ties), and for half i, cluster kk of nik > 1 members,
 * with a = its members among the half's first nf[i] - 1 entries (the reference leaves the last entry out of the numerator only):
 * ps = (#ordered pairs of a with equal classification, self-pairs included, - |a|) / (nik (nik - 1)); clusters of one member score 0.
 * prederr[(k - 2) * M + l] = (min ps[1,] + min ps[2,]) / 2; mean_pred[0] = 1 and mean_pred[k - 1] = R's mean() of the M values of k
 * (long double, two passes), k_max entries; *optimalk = the largest k with mean_pred[k - 1] > cutoff.  2 <= k_max < floor(n / 2),
 * M >= 1, 0 <= cutoff < 1.
 *
 * msnv_cluster_file -- the stage on files, computeClusters with its defaults: reads dist_path (<species>.filtered.mann.dist as
 * metaSNV_DistDiv.py --dist writes it; an NA or empty cell is MSNV_EFORMAT) and, when freq_path is not NULL, the *.filtered.freq
 * table; removes outliers (removeOutliersFromDistMatrixMinDissim, 3 sd, at most 5), writes <species>_freq_composition.tab and keeps the
 * samples whose 10/90 proportion is >= 0.8, picks the number of clusters by prediction strength (M = 50, up to 15 clusters of >= 3),
 * runs PAM, rates the stability of the number (>= 10 samples; stability_iters subsamples at each proportion, 10 / 5 there), drops
 * clusters under 3 members, and writes <prefix>_PS_values.tab, _distMatrixUsedForClustMedoidDefns.txt, _clustering.tab and
 * _clusNumStability.tab (prefix = <species>_mann) into out_dir, out_dir/noClustering/ (one cluster) or
 * out_dir/clustMedoidDefnFailed/.  Doubles are printed with %.15g.  result: [0] MSNV_CLUSTER_* [1] clusters [2] samples clustered
 * [3] outliers removed [4] stability score (1 Low, 2 Medium, 3 High; 0 not rated) [5] optimalk [6] PAM tasks run [7] 0.
 *
 * Randomness: R's generator is not reproduced.  With mix(x) = splitmix64's output function of state x + 0x9e3779b97f4a7c15
 * (z = x + 0x9e3779b97f4a7c15; z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9; z = (z ^ z >> 27) * 0x94d049bb133111eb; z ^ z >> 31), all mod 2^64:
 *   rand(seed, ordinal, i) = mix(mix(mix(seed) + ordinal) + i)
 *   permutation(seed, ordinal, n): p = 0..n-1; for i = n-1 down to 1: swap p[i], p[rand(seed, ordinal, i) mod (i + 1)]
 * The main run's permutation of (k, l) has ordinal (k - 2) * 50 + l.  Stability run r = 1 + 1024 * (index of the proportion) + iteration
 * draws its subsample as the first floor(n * prop) entries of permutation(seed, r << 32 | 0xffffffff, n) and the permutation of its
 * (k, l) with ordinal r << 32 | (k - 2) * 50 + l.  A draw depends on the seed and its ordinal alone, never on how tasks were batched. */
#define MSNV_CLUSTER_OK            0   /* two or more clusters, files in out_dir                                              */
#define MSNV_CLUSTER_NONE          1   /* one cluster: files in out_dir/noClustering/                                         */
#define MSNV_CLUSTER_MEDOID_FAILED 2   /* Gmax <= 1 ("Cluster medoid definition failed"): one cluster, matrix also in clustMedoidDefnFailed/ */
#define MSNV_CLUSTER_TOO_FEW       3   /* fewer than 6 samples with extreme SNV frequencies: only the composition file, in clustMedoidDefnFailed/ */
#define MSNV_CLUSTER_ALL_EQUAL     4   /* all remaining distances equal: likewise                                             */
typedef struct {
    uint64_t seed;
    double   ps_cut;            /* psCut, 0.8                                                   */
    int32_t  stability_iters;   /* clusNumStabilityIter, 10 (tests lower it); 1..1024           */
    int32_t  reserved;          /* 0                                                            */
} msnv_cluster_opts;
void msnv_cluster_opts_default(msnv_cluster_opts *o);
int msnv_pam_tasks(msnv_ctx *ctx, int32_t n, const double *dist, int64_t n_tasks, const int32_t *task_m, const int32_t *task_k,
                   const int32_t *idx, int32_t *medoids, int32_t *cluster, int32_t *n_swaps, double *ms_kernel);
int msnv_pred_strength(msnv_ctx *ctx, int32_t n, const double *dist, int32_t k_max, int32_t M, const int32_t *perms, double cutoff,
                       double *prederr, double *mean_pred, int32_t *optimalk, double *ms_kernel);
int msnv_cluster_file(msnv_ctx *ctx, const char *dist_path, const char *freq_path, const char *species, const char *out_dir,
                      const msnv_cluster_opts *opts, int64_t result[8], double *ms_kernel);
/* msnv_cluster_file_ex -- msnv_cluster_file with subpopr's -x / -y (clustering.R:43-51, computeSnvFreqStats.R:31-46).  In double, as R computes
 * them: h = x > 0.5 ? 1 - x : x; t = h * 100; hi = max(100 - t, t); lo = min(100 - t, t).  A sample is kept when #(cell < lo | cell > hi) / #covered
 * >= y on the table's cells as they are read (the kernel and strict count of msnv_freq_curves; 0 / 0 is not kept; a cell that is neither -1 nor
 * within [0, 100] is MSNV_EDOMAIN).  y <= 0 disables the filter: every sample left after outlier removal is used.  <species>_freq_composition.tab
 * keeps its three fixed columns.  x or y outside [0, 1], or NaN, is MSNV_EINVAL before any file is read.  filter NULL = the defaults, 0.1 and 0.8:
 * msnv_cluster_file is this call with filter NULL. */
typedef struct {
    double max_prop_reads_non_homog;   /* subpopr -x, 0.1 */
    double min_prop_homog_snv;         /* subpopr -y, 0.8 */
} msnv_cluster_filter;
void msnv_cluster_filter_default(msnv_cluster_filter *f);
int msnv_cluster_file_ex(msnv_ctx *ctx, const char *dist_path, const char *freq_path, const char *species, const char *out_dir,
                         const msnv_cluster_opts *opts, const msnv_cluster_filter *filter, int64_t result[8], double *ms_kernel);

/* The stability of each cluster's membership: getClusMembStability -> clusterAssignSubsample -> getClusMembStabScore
 * (src/subpopr/R/clusteringStability.R:129-148, :170-176, :224-237), i.e. fpc::clusterboot(bootmethod = "subset", clustermethod = claraCBI,
 * usepam = TRUE, dissolution = 0.5, recover = 0.75).  Restated from reading the R code and from memory of fpc; no R was run (DESIGN.md
 * section 7: unpinned).
 *
 * msnv_cluster_boot -- the array form.  dist: the n x n matrix, as for msnv_pam_tasks.  members: m sample indices, ascending: the clustered
 * samples.  1 <= k <= 32 and k < m.  Subset t is set_m[t] distinct positions 0..m-1 into the member list, in the order given, packed behind
 * each other in set_pos; k < set_m[t] <= m.  Anything else is MSNV_EDOMAIN or MSNV_EINVAL before any launch.  Out: cluster[m] (1..k) and
 * medoids[k], the PAM of the members in list order; and, for subset t re-clustered by PAM in its own order with the same k and every
 * original cluster j = 1..k, best_inter / best_union [t * k + j - 1]: over the new clusters c that have a member, ascending,
 *   inter = #(entries of the subset in j and in c), union = #(entries of the subset in j) + #(entries in c) - inter,
 * the FIRST c with the largest inter / union, fractions compared exactly as integers (a / b > c / d <=> a d > c b).  An original cluster
 * without an entry in the subset gets inter = 0; a union is never 0.  The Jaccard value is (double)inter / (double)union.  Two launches
 * for any number of subsets (at most 2^26 list entries in one call, else MSNV_ECAPACITY): the PAM kernel over the members and every
 * subset, then one workgroup per subset over the cluster ids the first left on the device.  A subset's result does not depend on its
 * place in the batch.
 *
 * msnv_membership_stability_file -- the stage on files.  dist_used_path: <species>_mann_distMatrixUsedForClustMedoidDefns.txt as
 * msnv_cluster_file writes it (write.table's form: n names in the header without a leading cell); all of its n samples are the members.
 * n < 10: MSNV_MEMBSTAB_NOT_RATED, nothing written.  Else 1 <= k <= 32 and k < n (MSNV_EDOMAIN).  The proportions and subset sizes are
 * those of msnv_cluster_file's number-stability run: low = max(0.3, ceil(10 / n * 10) / 10), prop = low + 0.1 pi while <= 1 + 1e-10, size =
 * min(n, floor(n prop)); subset b (0 <= b < boot_iters) of proportion pi is the first size entries of permutation(seed, 1 << 62 | pi << 32 |
 * b, n), in that order.  A proportion whose size is <= k is not clustered: its rows hold NA (R's pam stops there: a divergence).  Per
 * proportion and original cluster j, over the boot_iters values J_b = inter / union:
 *   clusterStabilityJaccardMean = R's mean();  clusterStabilityPropRecover = #(J_b >= 0.75) / #(J_b <= 0.5) as a double division (Inf for
 *   x / 0, NaN for 0 / 0): clusterboot's subsetrecover / subsetbrd, which is what the reference divides by.
 * Written into out_dir (%.15g, NaN, Inf, NA):
 *   <species>_mann_clusMembStability.tab   clusterID, nSamplesInCluster (of the original PAM partition), subsampleProp,
 *                                          clusterStabilityJaccardMean, clusterStabilityPropRecover; one row per (proportion, cluster)
 *   <species>_mann_stabilityAssessment.tab name, score: numClusters = getNClusStabScore of clus_num_stability_path (NA when NULL), then
 *                                          clust1..clustk = getClusMembStabScore: 1 + (recover@0.9 > 0.8 & jaccard@0.9 > 0.8) +
 *                                          (recover@0.7 > 0.9 & jaccard@0.7 > 0.9) with R's three-valued &, a NaN, NA or missing row
 *                                          being NA; Low, Medium, High or NA
 * result: [0] MSNV_MEMBSTAB_* [1] k [2] n [3] proportions [4] subsets clustered [5] the numClusters score (1..3, 0 = NA) [6] the lowest
 * cluster score (0 when any is NA) [7] 0. */
#define MSNV_MEMBSTAB_OK        0
#define MSNV_MEMBSTAB_NOT_RATED 1   /* fewer than 10 samples: the reference rates stability from 10 on */
typedef struct {
    uint64_t seed;
    int32_t  boot_iters;        /* clusterboot's B, 100 (tests lower it); 1..1024               */
    int32_t  reserved;          /* 0                                                            */
} msnv_membstab_opts;
void msnv_membstab_opts_default(msnv_membstab_opts *o);
int msnv_cluster_boot(msnv_ctx *ctx, int32_t n, const double *dist, int32_t m, const int32_t *members, int32_t k, int64_t n_sets,
                      const int32_t *set_m, const int32_t *set_pos, int32_t *medoids, int32_t *cluster, int32_t *best_inter,
                      int32_t *best_union, double *ms_kernel);
int msnv_membership_stability_file(msnv_ctx *ctx, const char *dist_used_path, const char *clus_num_stability_path, const char *species,
                                   int32_t k, const char *out_dir, const msnv_membstab_opts *opts, int64_t result[8], double *ms_kernel);

/* subpopr's computePCoA (src/subpopr/R/clustering.R:120-126, :472-505): ape::pcoa(correction = "none") of a species' distance matrix, the
 * numbers behind the ordination plots.  Restated from reading the R code and from memory of ape; no R was run (DESIGN.md section 7:
 * unpinned).  The eigen solver is hand-written and its result is a function of the matrix alone.
 *
 * msnv_pcoa -- the array form.  dist: the n x n matrix under msnv_pam_tasks' checks (2 <= n <= 4096, symmetric, zero diagonal, finite,
 * >= 0: else MSNV_EDOMAIN); 1 <= n_axes <= n (else MSNV_EINVAL).  Every operation is one fp64 operation, never contracted.
 *   centring   A_ij = -0.5 (d_ij d_ij); r_i = (sum of A_ij, j ascending) / n; g = (sum of r_i, i ascending) / n;
 *              B_ij = ((A_ij - r_i) - r_j) + g for i <= j, mirrored into j > i; trace = sum of B_ii, i ascending
 *   Jacobi     two-sided, cyclic, round-robin: m = n + (n & 1); a sweep is the steps r = 0..m-2; step r holds slot 0 = (m - 1, r) and slot
 *              i = ((r + i) mod (m - 1), (r - i) mod (m - 1)), i = 1..m/2-1, each ordered p < q; a slot that holds index n is the bye
 *              (one index).  A pair rotates when |a_pq| > tol = 2^-52 max |B_ij|: theta = (a_qq - a_pp) / (2 a_pq), t = (theta >= 0 ? 1
 *              : -1) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c; else t = 0, c = 1, s = 0.  All rotations of a
 *              step are applied together, block by block: the 2 x 2 block (rows of slot I, columns of slot J), I < J, becomes, columns
 *              first, x' = c_J x - s_J y, y' = s_J x + c_J y, then rows with c_I, s_I in the same form, and is written to itself and,
 *              transposed, to its mirror; the bye's blocks have one row and take the columns' rotation alone.  A pair's own block:
 *              a_pp - t a_pq, a_qq + t a_pq, a_pq = a_qp = 0 when it rotated.  V starts as I and takes the column form of every step.
 *              The solve ends after the first sweep in which no pair rotated; 64 sweeps without that are MSNV_EDOMAIN.
 *   output     eig[n]: the diagonal sorted descending (equal values in ascending diagonal position), |lambda| < sqrt(2^-52) set to 0;
 *              rel_eig = lambda / trace; axis_pct = max(lambda, 0) / (sum of max(lambda, 0) in sorted order) * 100 (getEig); k = the
 *              number of lambda > sqrt(2^-52); vectors row-major [n][n_axes]: column a < k is the eigenvector times sqrt(lambda_a),
 *              negated when its component of largest magnitude (the first of equals) is negative -- R's signs are LAPACK's accident --
 *              and a column a >= k is all NaN.
 * info: [0] MSNV_PCOA_* [1] sweeps [2] rotations applied [3] k [4] eigenvalues < -sqrt(2^-52) [5..7] 0.
 *
 * msnv_pcoa_file -- the stage on files.  Reads dist_path (<species>.filtered.mann.dist, as msnv_cluster_file does), removes outliers by
 * the same routine and ordinates the remaining samples with two axes.  dir is msnv_cluster_file's out_dir or its noClustering/: clust
 * comes from dir/<species>_mann_clustering.tab (a sample it does not list: NA), propFreqHomog from the freq_data_sample_10_90 column of
 * dir/<species>_freq_composition.tab (NA when the file is absent or does not list the sample).  Written into dir, as write.table(sep =
 * '\t', quote = F) prints them, doubles with %.15g:
 *   <species>_mann_pcoa_proj.tab   Axis.1, Axis.2, propFreqHomog, clust; one row per sample.  Not written on MSNV_PCOA_TOO_FEW_AXES, the
 *                                  reference's "Error during pcoa"
 *   <species>_mann_pcoa_eig.tab    Eigenvalues, Relative_eig, axisPercent; rows 1..n.  Our own file: the reference keeps these numbers
 *                                  for the axis labels of its plots only
 * result: info's [0..4], then [5] samples ordinated [6] outliers removed [7] 0. */
#define MSNV_PCOA_OK            0
#define MSNV_PCOA_TOO_FEW_AXES  1   /* k < 2 */
int msnv_pcoa(msnv_ctx *ctx, int32_t n, const double *dist, int32_t n_axes, double *eig, double *rel_eig, double *axis_pct, double *vectors,
              int64_t info[8], double *ms_kernel);
int msnv_pcoa_file(msnv_ctx *ctx, const char *dist_path, const char *dir, const char *species, int64_t result[8], double *ms_kernel);

/* The row order of the four distance heatmaps of subpopr's per-species report (src/subpopr/inst/rmd/detailedSpeciesReport.rmd:142, :222, :250,
 * :402): heatmap(distfun = as.dist, hclustfun = hclust(method = ...)).  Restated from memory of R's hclust.f, hcass2, as.dendrogram.hclust,
 * reorder.dendrogram and heatmap; no R was run (unpinned).
 *
 * msnv_hclust_tasks -- the array form.  dist: the n x n matrix under msnv_pam_tasks' checks (else MSNV_EDOMAIN).  A task is a list of m distinct
 * sample indices (2 <= m <= n; a repeated or outlying index: MSNV_EDOMAIN) and a method (not one of MSNV_HCLUST_*, or n_tasks < 1: MSNV_EINVAL);
 * the lists are packed behind each other in idx, at most 2^26 entries in one call (MSNV_ECAPACITY).  Positions 0..m-1 are positions in the
 * list: W[a][b] = D[idx[a]][idx[b]], size[a] = 1, every position active.
 *   step s = 1..m-1   among the active pairs a < b the smallest W[a][b]; among equal values the smallest a, then the smallest b; h_s = W[a][b].
 *              For every other active k: W[k][a] = W[a][k] = f(W[k][a], W[k][b]) with f(x, y) =
 *                MSNV_HCLUST_AVERAGE   (size[a] x + size[b] y) / (size[a] + size[b]), sizes as doubles: two products, one sum, one quotient
 *                MSNV_HCLUST_COMPLETE  max(x, y)          MSNV_HCLUST_SINGLE  min(x, y)          MSNV_HCLUST_MCQUITTY  0.5 x + 0.5 y
 *              each one fp64 operation, never contracted.  Then size[a] += size[b] and b is inactive.  All four are monotone: h_1 <= ... <= h_{m-1}.
 *   merge      R's hc$merge: a singleton is -(position + 1), the cluster made at step s is s; row s holds the labels of the clusters at a and
 *              at b -- two singletons in the order (a, b), a singleton before a cluster, of two clusters the smaller step first
 *   height     height[s - 1] = h_s
 *   order      R's hc$order, as 0-based positions: the leaves of the tree left to right, row s's first entry the left child
 * With off_t the sum of the earlier m: task t's merge is 2 (m_t - 1) ints (row by row) at 2 (off_t - t), its height m_t - 1 doubles at
 * off_t - t, its order m_t ints at off_t.  One workgroup per task in one launch; a batch whose gathered sub-matrices (8 m^2 bytes each) pass the
 * scratch budget is cut into several launches.  The result is a function of the task alone.
 * Known divergence: R finds the minimum through nearest-neighbour lists that it repairs lazily; when an update creates a value equal to a row's
 * current nearest distance at a smaller column index, R keeps the old column and this rule takes the new one.  Without equal cells among the
 * candidates the two agree.
 *
 * msnv_heatmap_order -- reorder(as.dendrogram(hc), weights) with agglo.FUN = sum, then order.dendrogram; host only, no context.  A leaf's value is
 * its weight; at every node, bottom up, the two children are put in ascending order of value (equal values keep their merge order) and the node's
 * value is the long double sum of the two in that order, rounded to double.  order: the leaves left to right, 0-based positions.  m < 2 or a
 * merge that is not a tree in the encoding above: MSNV_EINVAL; a weight that is not finite: MSNV_EDOMAIN.
 *
 * msnv_heatmap_file -- the stage on files.  Reads dist_path (<species>.filtered.mann.dist, as msnv_cluster_file does; an NA or empty cell is
 * MSNV_EFORMAT) and the sample names in the header of dir/<species>_mann_distMatrixUsedForClustMedoidDefns.txt -- the discovery subset, whose
 * cells are taken from dist_path; a name dist_path does not hold, or one listed twice: MSNV_EFORMAT -- and clust from
 * dir/<species>_mann_clustering.tab (the file absent or a sample not listed: NA).  Both trees run in one call of the array form: every sample
 * with MSNV_HCLUST_AVERAGE (:142, :222, :402), the discovery subset with MSNV_HCLUST_COMPLETE (:250).  The weights are R's rowMeans of the tree's
 * sub-matrix: a long double sum over ascending columns, divided by m, rounded to double.  Written into dir, as write.table(sep = '\t', quote = F)
 * prints them, doubles with %.15g (our own files: the reference keeps these numbers as pixels only):
 *   <species>_mann_hclust_{all,discovery}.tab    merge1, merge2, height; rows 1..m-1
 *   <species>_mann_heatmap_{all,discovery}.tab   one row per sample in heatmap order, named by the sample: index (1-based place in the tree's
 *                                                sample list), hclustPos (1-based place in hc$order), inDiscoverySubset (TRUE / FALSE), clust
 * result: [0] MSNV_HEATMAP_* (NO_DISCOVERY: the medoid-definition file is absent or names fewer than two samples; the two _all files are
 * written) [1] samples in the full tree [2] samples in the discovery tree [3] 1 when a clustering file was read [4..7] 0. */
#define MSNV_HCLUST_AVERAGE   0
#define MSNV_HCLUST_COMPLETE  1
#define MSNV_HCLUST_SINGLE    2
#define MSNV_HCLUST_MCQUITTY  3
#define MSNV_HEATMAP_OK            0
#define MSNV_HEATMAP_NO_DISCOVERY  1
int msnv_hclust_tasks(msnv_ctx *ctx, int32_t n, const double *dist, int64_t n_tasks, const int32_t *task_m, const int32_t *task_method, const int32_t *idx,
                      int32_t *merge, double *height, int32_t *order, double *ms_kernel);
int msnv_heatmap_order(int32_t m, const int32_t *merge, const double *weights, int32_t *order);
int msnv_heatmap_file(msnv_ctx *ctx, const char *dist_path, const char *dir, const char *species, int64_t result[8], double *ms_kernel);

/* The numbers behind the two SNV-frequency plots of subpopr's per-species report (src/subpopr/R/snvFreqPlot.R:1-113, drawn by defineSubpopulations,
 * profileSubpops.R:152-158; shown by detailedSpeciesReport.rmd:176-212), and the band the clustering's sample selection applies
 * (clustering.R:43-51, computeSnvFreqStats.R:31-46).  Restated from reading the R code; no R was run (unpinned).
 *
 * msnv_freq_curves -- the array form.  rows: host memory, row-major [n_pos][n_samples], on the percent scale, NaN for a cell without coverage.
 * n_samples >= 1, n_pos >= 0 (else MSNV_EINVAL; n_pos = 0 gives all zeros); a NaN band is MSNV_EINVAL.  counts: uint64 [n_samples][102]:
 *   [k], k = 0..49   cells <= k                      [50 + k]   cells >= 100 - k
 *   [100]            covered (non-NaN) cells         [101]      cells < strict_lo or > strict_hi
 * A cell that is neither NaN nor within [0, 100] is MSNV_EDOMAIN (R would count a stray negative cell as low: a divergence).  The counts are
 * integers summed with integer atomics: they do not depend on the grid, on the slab cuts (MSNV_STAGE_SLAB_ROWS) or on the order of the blocks.
 * The table goes to the device in row slabs, so it may be larger than device memory.  *ms_kernel: the kernel's time by events, summed over the slabs.
 * msnv_freq_curves_geometry: the rows and the sample columns one block of the kernel covers (for tests that sit on those seams).
 *
 * msnv_freq_bands -- computeSnvFreqStats (computeSnvFreqStats.R:1-24) on the same arrays, the kernel msnv_cluster_file counts with.  counts: uint64
 * [n_samples][4]: cells < 20 or > 80, < 10 or > 90, < 5 or > 95, covered cells.  No domain check.  The yardstick profiles/snvfreq_time.py holds
 * msnv_freq_curves against.
 *
 * msnv_snvfreq_file -- the stage on files.  freq_path: the *.filtered.freq table on metaSNV's [0, 1] scale (-1 and NA: no coverage); a cell above 1 is
 * MSNV_EDOMAIN with the reference's message (profileSubpops.R:145-147), any other cell outside [0, 1] MSNV_EDOMAIN; cells are then multiplied by 100
 * in double.  opts NULL: the defaults; a value outside [0, 1] or a reserved field that is not 0: MSNV_EINVAL.  With x = max_prop_reads_non_homog, y =
 * min_prop_homog_snv, n the covered cells of a sample and N the rows, every quotient one double division of two integers (n = 0: NaN):
 *   cutoffIndex = 1..50, k = cutoffIndex - 1:  propLow = #(cell <= k) / n, propHigh = #(cell >= 100 - k) / n, propSuffCov = n / N, propPass = propLow +
 *     propHigh; sampleUsedForMedoidDefn = NA unless (double)cutoffIndex == x * 100 + 1 as computed in double (0.07: index 8; 0.29: 29.999999999999996,
 *     no index), there propPass > y, NA when propPass is NaN
 *   h = x > 0.5 ? 1 - x : x, t = h * 100, hi = max(100 - t, t), lo = min(100 - t, t):  propHomogStrict = #(cell < lo | cell > hi) / n;
 *     selectedForDiscovery = propHomogStrict >= y (NaN: FALSE) -- the rule computeClusters selects samples by; it differs from the plot's in all
 *     three comparisons
 * Written into out_dir/snvFreqPlots/ (both created when missing), as write.table(sep = '\t', quote = F, row.names = F) prints them: doubles with
 * %.15g, NaN, logicals TRUE / FALSE / NA (our own files: the reference keeps these numbers as pixels only; the histogram's bins are not written):
 *   <species>_snvFreq_cutoffs.tab   cutoffIndex, sampleID, propLow, propHigh, propSuffCov, propPass, sampleUsedForMedoidDefn; expand.grid order:
 *                                   samples in column order, cutoffIndex 1..50 within a sample
 *   <species>_snvFreq_fixed.tab     sampleID, propPass, propSuffCov, sampleUsedForMedoidDefn (the first file's row at the matching cutoffIndex; NA, NA,
 *                                   NA when none matches), propHomogStrict, selectedForDiscovery; one row per sample
 * result: [0] samples [1] rows [2] the matching cutoffIndex or 0 [3] samples with sampleUsedForMedoidDefn TRUE [4] samples selectedForDiscovery
 * [5] samples without a covered cell [6], [7] 0. */
typedef struct {
    double  max_prop_reads_non_homog;   /* subpopr -x fixReadThreshold, 0.1; 0..1                     */
    double  min_prop_homog_snv;         /* subpopr -y fixSnvThreshold, 0.8; 0..1                      */
    int32_t reserved[2];                /* 0                                                          */
} msnv_snvfreq_opts;
void msnv_snvfreq_opts_default(msnv_snvfreq_opts *o);
void msnv_freq_curves_geometry(int32_t *rows_per_block, int32_t *columns_per_block);
int msnv_freq_curves(msnv_ctx *ctx, const double *rows, int64_t n_pos, int32_t n_samples, double strict_lo, double strict_hi, uint64_t *counts, double *ms_kernel);
int msnv_freq_bands(msnv_ctx *ctx, const double *rows, int64_t n_pos, int32_t n_samples, uint64_t *counts, double *ms_kernel);
int msnv_snvfreq_file(msnv_ctx *ctx, const char *freq_path, const char *species, const char *out_dir, const msnv_snvfreq_opts *opts, int64_t result[8],
                      double *ms_kernel);

/* subpopr's writeGenotypeFreqs -> computeUniquePosPerCluster (src/subpopr/R/writeGenotypeFreqs.R:2-112, :195-277): which SNVs tell one
 * subspecies from every other.  Restated from reading the R code; no R was run (unpinned).
 *
 * msnv_genotype_rows -- the rule on arrays.  rows: host memory, row-major [n_pos][n_samples], NaN for no coverage, scaled to 0..100.
 * clust[s]: 0 for a column not in use, or 1..n_clusters.  2 <= n_clusters <= 32, 1 <= n_samples <= 65536, every cluster has a column,
 * every non-NaN cell lies in [0, 100]: anything else is MSNV_EDOMAIN.  For row p and cluster i, with C_i the columns of cluster i, N_i the
 * in-use columns outside it and na(X) the NaN cells of the row over X, bit i - 1 of select_mask[p] is set when
 *   1. (double)na(C_i) / |C_i| < 0.2
 *   2. (double)na(N_i) / |N_i| < 0.2
 *   3. for every other cluster j: |mean(C_i) - mean(C_j)| > threshold, strictly; means over the non-NaN cells, a cluster without one
 *      gives a difference of 0
 * and bit i - 1 of flip_mask[p] is set where the select bit is and, among the non-NaN cells of C_i, more are < 50 than >= 50
 * (majorAllel(...) == 0, computeSnvFreqStats.R:48-57: the median of a 0 / 1 vector is 0 exactly when the zeros outnumber the ones).
 * The means of condition 3 are R's rowMeans: a long double sum in ascending column order over the count, rounded to double.  The kernel
 * sums in fp64 in its own order, which is off by at most n * 100 * 2^-53 < 7.3e-10 per mean (cells in [0, 100], n <= 65536), under 2e-9
 * for a difference of two; every row with a comparison within 1e-6 of the threshold is redone on the host by the long double rule and
 * *n_rechecked counts those rows.  The masks are therefore the long double rule's on every row.  The table goes to the device in slabs,
 * so it may be larger than device memory.  *ms_kernel: the kernel's time by events, summed over the slabs.
 *
 * msnv_genotype_file -- the stage on files.  freq_path: the *.filtered.freq table (a non-NaN cell above 1 is MSNV_EDOMAIN; cells are then
 * multiplied by 100).  clustering_path: <species>_mann_clustering.tab as msnv_cluster_file writes it (a header "clust", then
 * name<TAB>integer; anything else is MSNV_EFORMAT).  0 < uniq_threshold < 1 (uniqSubpopSnvFreqThreshold, 0.8).  The samples in use are the
 * freq columns the clustering lists, in freq column order; the clusters are numbered by first appearance in that order.  Written into
 * out_dir (created if missing): <species>_hap_out.txt, per cluster with positions <species>_<id>_hap_positions.tab (header posId<TAB>flip,
 * rows counter<TAB>row label<TAB>TRUE|FALSE in table order), and on MSNV_GENOTYPE_OK <species>_hap_freq_mean.tab and _median.tab: per
 * cluster and per sample in use, R's mean() and median() over that cluster's selected rows, flipped rows as 100 - x, NA skipped (%.15g).
 * result: [0] MSNV_GENOTYPE_* [1] clusters [2] samples in use [3] table rows [4] genotyping positions over all clusters [5] rows
 * rechecked on the host [6] nCorrAssign [7] good samples. */
#define MSNV_GENOTYPE_OK              0   /* every cluster has positions and the samples' summed medians are coherent            */
#define MSNV_GENOTYPE_SINGLE          1   /* one distinct cluster or none: "Single cluster", no kernel runs                      */
#define MSNV_GENOTYPE_NO_POSITIONS    2   /* no cluster has a genotyping position                                                */
#define MSNV_GENOTYPE_CLUSTER_MISSING 3   /* at least one cluster has none                                                       */
#define MSNV_GENOTYPE_CUTOFF_BAD      4   /* more than 15 % of the samples sum to > 120 or < 80 over their cluster medians       */
int msnv_genotype_rows(msnv_ctx *ctx, uint64_t n_pos, int32_t n_samples, const double *rows, const int32_t *clust, int32_t n_clusters,
                       double threshold, uint32_t *select_mask, uint32_t *flip_mask, uint64_t *n_rechecked, double *ms_kernel);
int msnv_genotype_file(msnv_ctx *ctx, const char *clustering_path, const char *freq_path, const char *species, const char *out_dir,
                       double uniq_threshold, int64_t result[8], double *ms_kernel);

/* subpopr's useGenotypesToProfileSubpops -> writeSubpopsForAllSamples (src/subpopr/R/profileSubpops.R:228-274, writeSubpopsForAllSamples.R) and
 * useSpeciesAbundToCalcSubspeciesAbund -> writeSubpopAbundSpeciesAbund (profileSubpops.R:277-310, writeSubpopAbund.R:99-169): how abundant each
 * subspecies is in every sample metaSNV was run on.  Restated from reading the R code; no R was run (unpinned).
 *
 * msnv_subpop_profile_columns -- the kernel on arrays.  rows: host memory, row-major [n_rows][n_samples], NaN for no coverage, every other cell
 * within [0, 100] (else MSNV_EDOMAIN); flip: one byte per row, a row with a non-zero byte counts as 100 - x (the fp64 subtraction R does).
 * 1 <= n_samples <= 65536 and 1 <= n_rows <= 2^31 - 1, else MSNV_EDOMAIN.  Per column s, over its called (non-NaN) cells: n_called, n_gt0 (> 0),
 * n_ge5 (>= 5), n_eq0 (== 0), n_eq100 (== 100), and mid_lo / mid_hi, the order statistics of 0-based ranks (n - 1) / 2 and n / 2 (integer
 * division): equal when n is odd, NaN when n is 0, otherwise values that occur in the column, bit for bit (-0.0 counts as +0.0).  Everything is
 * exact; median(x) is mean({mid_lo, mid_hi}).  The matrix goes to the device in bands of columns: cols_per_pass = 0 sizes a band from half of
 * the free device memory, a positive value forces that width.  *ms_kernel: the kernel's time by events, summed over the bands.
 *
 * msnv_subpop_profile_files -- writeSubpopsForAllSamples on files.  Sample names: the basenames of the lines of all_samples_path, in order.
 * Cluster files: <out_dir>/<species>_*.pos.freq in byte order of their names (msnv_snv_allele_freq writes them: id contig:ann:pos:base, then one
 * cell per sample, -1 = NA; another column count is MSNV_EFORMAT); the cluster number is the text between the last '_' and the first '.' of the
 * name (not an integer: MSNV_EFORMAT), and <out_dir>/<species>_<cluster>_hap_positions.tab (as msnv_genotype_file writes it) lists the cluster's
 * positions and flips.  Ids are matched as contig:pos:base; a duplicate id in either file is MSNV_EFORMAT; a listed position the .pos.freq lacks
 * is one all-NA row.  With G listed positions a sample is kept when n_called >= max_prop_uncalled * G (fp64 product; 0 < max_prop_uncalled <= 1,
 * else MSNV_EDOMAIN); a cluster with fewer than two kept samples is skipped.  Written into out_dir, every file as write.table(sep = '\t',
 * quote = F) prints it with %.15g: <species>_extended_clustering_abundanceSummaryStats.tsv (per usable cluster and kept sample: Sample, Cluster,
 * mean, median, standardDeviation, prevalence, prevalenceGte5, n0, n100, nNoCoverage; mean and sd by R's long double rules on the host),
 * _wFreq_unfiltered.tab (the samples with a median in every usable cluster, a column of medians per cluster), _wFreq.tab (those whose long double
 * row sum lies in [80, 120], minus the samples with median > 30 and prevalence < 0.75 in any cluster), _clustering.tab (column "clust": the
 * 1-based position of the single median above min_genotype_abundance, else NA) and lines appended to _stat.txt.  When the first usable cluster
 * is not cluster 1, or no sample has a median in every usable cluster, R binds columns of different samples: the summary table is written and
 * the call returns MSNV_EDOMAIN.  result: [0] MSNV_PROFILE_* [1] cluster files found [2] usable [3] samples in the unfiltered table [4] in the
 * filtered one [5] rejected for their sum [6] rejected as bad [7] assigned a cluster.
 *
 * msnv_subpop_abundance_files -- writeSubpopAbundSpeciesAbund on files; host only.  Reads <out_dir>/<species>_extended_clustering_wFreq.tab
 * (numeric headers get R's X prefix) and the species abundance table ('#' lines skipped; first line: a corner cell and the sample names; first
 * column: species), takes the samples both hold in the table's column order (none, and a suffix given: retried with the suffix appended to the
 * table's names), and writes freq / 100 * abundance to <species>_allClust_relativeAbund.tab and, per column x = 1.., to
 * <species>_clust_<x>_hap_coverage_extended_normed.tab.  Species absent or listed twice, no frequency rows, no shared sample: MSNV_EDOMAIN with
 * R's text.  counts: samples used, clusters, samples in wFreq.tab, sample columns of the abundance table. */
#define MSNV_PROFILE_OK          0   /* the five files are written                                                                      */
#define MSNV_PROFILE_NO_FILES    1   /* no <species>_*.pos.freq: "0/0 clusters had usable placing data." appended to _stat.txt          */
#define MSNV_PROFILE_NONE_USABLE 2   /* no cluster has two kept samples: "0/<n> clusters ..." appended, nothing else written             */
int msnv_subpop_profile_columns(msnv_ctx *ctx, int64_t n_rows, int32_t n_samples, const double *rows, const uint8_t *flip, int32_t cols_per_pass,
                                uint32_t *n_called, uint32_t *n_gt0, uint32_t *n_ge5, uint32_t *n_eq0, uint32_t *n_eq100, double *mid_lo,
                                double *mid_hi, double *ms_kernel);
int msnv_subpop_profile_files(msnv_ctx *ctx, const char *species, const char *out_dir, const char *all_samples_path, double max_prop_uncalled,
                              double min_genotype_abundance, int64_t result[8], double *ms_kernel);
int msnv_subpop_abundance_files(const char *species, const char *out_dir, const char *abundance_path, const char *sample_suffix,
                                uint64_t counts[4]);

/* ------------------------------------------------------------------------------------
 * Staged form of the same path.
 * ------------------------------------------------------------------------------------ */

/* Reference description: contigs in BAM-header order.  seqs[i] may be NULL (contig absent
 * from the FASTA: mpileup then prints 'N').  The library copies everything. */
typedef struct {
    int32_t            n_contigs;
    const char *const *names;
    const int64_t     *lengths;    /* @SQ LN                                   */
    const char *const *seqs;       /* FASTA characters, case preserved, or NULL */
    const int64_t     *seq_lens;
} msnv_ref_desc;

/* ctx may be NULL: the dataset then serves the host-stage entry points only (add_sample_*, pileup_qualities,
 * sample_stats, first_lines) and msnv_dataset_finalize fails with MSNV_ENODEV -- nothing is ever computed on the CPU. */
int  msnv_dataset_create(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params,
                         msnv_dataset **out);
/* Convenience: contigs from the header of `bam_path`, sequences from `fasta_path`. */
int  msnv_dataset_create_from_files(msnv_ctx *ctx, const char *bam_path, const char *fasta_path,
                                    const msnv_params *params, msnv_dataset **out);
/* Gives a dataset that was created without a context (ctx = NULL: host-stage entry points only) its device, before msnv_dataset_finalize.
 * A one-shot driver creates the HIP context (~0.5 s of runtime start-up) on a thread of its own while the BAMs are read, inflated and
 * packed by the host threads (metasnv_amd/cli.py); the reference's counterpart is process start-up of its tools. */
int  msnv_dataset_attach_ctx(msnv_dataset *ds, msnv_ctx *ctx);
void msnv_dataset_destroy(msnv_dataset *ds);

/* msnv_mpileup_text  <-  samtools mpileup -f ref_fasta [-l bed_split_path] -B -b <bam list> [-q -Q -A -x -d --ff] > out_path
 * (metaSNV.py:160-165, the left half of its pipe): the pileup TEXT itself, the reference's process boundary between samtools and
 * snpCall, formatted on the device (csrc/mptext_k.hip) -- one line `name \t pos \t REF { \t cnt \t bases \t quals }` per position
 * that a read passing the filters covers, samples in bam_paths order, elements in file order ([^ mapq] base | * | > < [+n ins | -n del]
 * [$]; bam_plcmd.c pileup_seq [EXT]).  -B is implied: base qualities are never recomputed (no BAQ).
 *   out_path NULL or "-": stdout.  Of params only the mpileup fields are read (min_baseq -Q, flag_filter --ff, count_orphans -A,
 *   max_depth -d, min_mapq -q, ignore_overlaps -x).
 *   stats (may be NULL): [0] lines, [1] samples, [2] text bytes, [3] pileup elements printed, [4] measure-pass kernel ms,
 *   [5] write-pass kernel ms, [6] batches of text that left the device (MSNV_MPTEXT_BATCH bytes each at most, whole tiles),
 *   [7] rounds of samples that went up (MSNV_MPTEXT_ROUND each).
 * DESIGN.md section 7 lists the one divergence from samtools' text (the quality character of a deletion / ref-skip element of the
 * first mate in front of an overlap).
 * msnv_mpileup_text(ctx, args, stats) is msnv_mpileup_text_ex(ctx, args, NULL, stats). */
typedef struct {
    const char *const *bam_paths;
    int32_t     n_bams;
    const char *ref_fasta;        /* -f; NULL: every reference character is N              */
    const char *bed_split_path;   /* -l or NULL                                            */
    const char *out_path;         /* stdout of samtools                                    */
    int32_t     host_threads;     /* BAM decode / pre-pass threads, 0 = auto               */
    msnv_params params;
} msnv_mpileup_text_args;
int msnv_mpileup_text(msnv_ctx *ctx, const msnv_mpileup_text_args *args, uint64_t stats[8]);
/* msnv_mpileup_text_opts  <-  samtools mpileup -a / -aa, -s (--output-MQ), -O (--output-BP) (samtools >= 1.10 bam_plcmd.c [EXT],
 * unpinned like the rest of SURVEY.md Appendix C: restated from the manual and from memory of the source, no samtools binary was run
 * against them).  With them a line is `name \t pos \t REF { \t cnt \t bases \t quals [\t MQ] [\t BP] }`:
 *   MQ: one character min(mapq + 33, 126) per element the bases column keeps, in its order (the character behind a `^`);
 *   BP: the 1-based offset in the read, qpos + 1, of every kept element, joined by `,` (deletion / ref-skip element: the read
 *       bases consumed before it; not strand-aware, not clamped for a read without SEQ);
 *   a cell without kept elements prints `0 \t * \t *` and `\t *` per extra column.
 *   all_positions 1: a zero-depth line as well for every other position of every contig that prints a line without it -- 1 to the
 *   contig's @SQ length, cut to the contig's -l region; REF is the FASTA character, N beyond the FASTA or without a FASTA record.
 *   all_positions 2: the same for every contig of the header, reads or none (with -l: the listed regions).
 * Every field 0 (msnv_mpileup_text_opts_default) or opts = NULL: the text of msnv_mpileup_text, byte for byte.  all_positions outside
 * 0..2 or reserved != 0: MSNV_EINVAL. */
typedef struct {
    int32_t all_positions;   /* 0 = lines under reads only, 1 = -a, 2 = -aa               */
    int32_t output_mq;       /* -s: a MAPQ column behind the qualities                     */
    int32_t output_bp;       /* -O: a read-offset column behind that                       */
    int32_t reserved;        /* 0                                                          */
} msnv_mpileup_text_opts;
void msnv_mpileup_text_opts_default(msnv_mpileup_text_opts *o);
int  msnv_mpileup_text_ex(msnv_ctx *ctx, const msnv_mpileup_text_args *args, const msnv_mpileup_text_opts *opts, uint64_t stats[8]);
/* The same text from record streams in memory (what sam_read1() yields, one stream per sample; the reference as msnv_ref_desc,
 * the -l regions as for msnv_dataset_set_bed: at most one per contig, n_bed = 0 for none).  *text is released with msnv_free;
 * the text is not NUL-terminated.  What the tests and the Python layer use. */
int msnv_mpileup_text_records(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params, int32_t n_bed, const int32_t *bed_tid,
                              const int64_t *bed_beg, const int64_t *bed_end, const uint8_t *const *records, const uint64_t *n_bytes,
                              int32_t n, char **text, uint64_t *text_bytes, uint64_t stats[8]);
/* msnv_mpileup_text_records with options behind `params` (NULL: none; msnv_mpileup_text_records is this call with opts = NULL). */
int msnv_mpileup_text_records_ex(msnv_ctx *ctx, const msnv_ref_desc *ref, const msnv_params *params, const msnv_mpileup_text_opts *opts,
                                 int32_t n_bed, const int32_t *bed_tid, const int64_t *bed_beg, const int64_t *bed_end,
                                 const uint8_t *const *records, const uint64_t *n_bytes, int32_t n, char **text, uint64_t *text_bytes,
                                 uint64_t stats[8]);
/* The sizes at which the kernels' forms change (tests): positions per tile, read descriptors taken through LDS at a time. */
void msnv_mpileup_text_geometry(int32_t *tile_positions, int32_t *lds_reads);

/* Restrict the shard: BED regions (mpileup -l; 0-based half-open, at most one region per
 * contig) and/or a contig mask.  Must precede the first add_sample call. */
int  msnv_dataset_set_bed(msnv_dataset *ds, int32_t n, const int32_t *tid, const int64_t *beg, const int64_t *end);
int  msnv_dataset_set_bed_file(msnv_dataset *ds, const char *bed_path);
int  msnv_dataset_set_contig_mask(msnv_dataset *ds, const uint8_t *mask, int32_t n);

/* Append one sample (= one BAM of all_samples), in order.  `records` = concatenated raw
 * uncompressed BAM alignment records (each starting with its int32 block_size), i.e. what
 * sam_read1() yields (qaCompute.cpp:441). */
int  msnv_dataset_add_sample_records(msnv_dataset *ds, const uint8_t *records, uint64_t n_bytes);
/* n record streams appended as n samples, in order, packed by a pool of host_threads threads (0 = all cores): what the N-rank
 * driver does with the streams of one exchange round (metasnv_amd/parallel.py: feed_sharded). */
int  msnv_dataset_add_sample_records_many(msnv_dataset *ds, const uint8_t *const *records, const uint64_t *n_bytes, int32_t n, int32_t host_threads);
/* The same for record streams that already lie in the HBM of the dataset's device -- what an all-to-all over RCCL has just received
 * (metasnv_amd/parallel.py: exchange_records), what the device inflate has written: the records never visit a host core.  The per-read
 * stage of both reference tools runs as kernels over them (csrc/devscan.hip, csrc/devpack.hip): record boundaries, the read loop and CIGAR walk of
 * qaCompute (qaCompute.cpp:441-593) and, for `samtools mpileup` (metaSNV.py:160-165), its read filters, the CIGAR walk to aligned
 * segments and the -Q test of every base.  The streams are copied; the caller may release them when the call returns.
 * Every add_sample_* entry point takes this route when the dataset has a device context (MSNV_PACK=host keeps the stage on the
 * host threads: pack.cpp, the same bytes).  The three sequential edits -- depth cap, overlapping-mate tweak, snpCall's token
 * limit -- are a host pre-pass over the samples whose records can trigger them. */
int  msnv_dataset_add_sample_records_device(msnv_dataset *ds, const void *const *dev_records, const uint64_t *n_bytes, int32_t n);
/* ... and WITHOUT the copy (round 5), for streams that lie in ONE device buffer the caller hands over for the duration of the call:
 * stream i = bytes [offsets[i], offsets[i] + n_bytes[i]) of `dev_buffer` (capacity bytes).  The buffer must start on 16 bytes and hold
 * at least 256 readable bytes behind the last stream's end (the kernels read whole 16-byte pieces around a record); the streams must not
 * overlap and must come in ascending order.  The library reads the records where they lie and MAY EDIT base qualities in place (htslib's
 * overlapping-mate tweak, snpCall's token limit: what the reference tools do to their own copy of a record, sam.c [EXT],
 * call_vC.cpp:481-483).  The last kernels of the call may still be READING the buffer when it returns (the host goes on with the
 * tile index meanwhile): the buffer is the library's -- valid, not written by anyone else -- until the NEXT call on this dataset that
 * adds samples, finalizes or destroys it has returned.  What the device inflate leaves in HBM goes this way, and the bench's "records
 * resident in HBM -> calls" region starts here. */
int  msnv_dataset_add_sample_records_resident(msnv_dataset *ds, void *dev_buffer, uint64_t capacity, const uint64_t *offsets, const uint64_t *n_bytes, int32_t n);
int  msnv_dataset_add_sample_bam(msnv_dataset *ds, const char *bam_path);
/* Decode many BAMs with a host thread pool, preserving order. */
int  msnv_dataset_add_sample_bams(msnv_dataset *ds, const char *const *bam_paths, int32_t n, int32_t host_threads);

/* The files are read, inflated and checked now (host threads), packed by msnv_dataset_finalize: a dataset created without a context
 * (msnv_dataset_attach_ctx later) still gets the per-read stage as kernels.  No other add_sample_* call may follow: every one of them
 * returns MSNV_EINVAL on a dataset that holds staged streams (more staging is fine).
 * Failure of any add_sample_* call leaves the dataset as it was before the call -- except when the call had already packed part of its
 * samples on the device (a later round of the same call failed: out of memory, a malformed record): such a dataset answers MSNV_EINVAL
 * to every further add_sample_* and to msnv_dataset_finalize and can only be destroyed. */
int  msnv_dataset_stage_sample_bams(msnv_dataset *ds, const char *const *bam_paths, int32_t n, int32_t host_threads);

/* Host-stage seam (tests, A/B against `samtools mpileup` text): writes to `out` (n_bytes) the same record stream with the
 * base qualities as the pileup engine sees them -- after the overlapping-mate tweak (unless params.ignore_overlaps) and
 * with the bases behind params.token_limit characters of a sample's base string set to quality 0 -- under this dataset's
 * read filters, BED and contig mask.  Does not add a sample.  (With params.min_baseq = 0 a quality of 0 is not below the
 * cutoff, so this FORM cannot tell a cut base from a counted one; the dataset itself marks cut bases below every cutoff:
 * pack.cpp QUAL_CUT.) */
int  msnv_dataset_pileup_qualities(const msnv_dataset *ds, const uint8_t *records, uint64_t n_bytes, uint8_t *out);

/* Builds the tile index and uploads the packed columns to HBM. */
int  msnv_dataset_finalize(msnv_dataset *ds);

typedef struct {
    uint64_t n_samples, n_contigs, n_positions;   /* positions = sum of shard contig lengths      */
    uint64_t n_reads, n_reads_pileup;             /* stored reads / reads that pass mpileup filters */
    uint64_t n_pileup_bases;                      /* (read, ref position) pairs from M/=/X ops of
                                                     reads that pass the read-level filters        */
    uint64_t bytes_headers, bytes_cigar, bytes_seq, bytes_qual, bytes_ref, bytes_index;
    uint64_t n_tiles, n_pairs, n_work;
    uint64_t device_bytes;                        /* total HBM held by the dataset                 */
    uint64_t allele_planes;                       /* 1: the per-sample allele counts go through byte planes (noisy reads), 0: through
                                                     sparse events (clean reads); picked by finalize from the sampled mismatch rate */
    uint64_t sampled_mismatch_ppm;                /* aligned bases that differ from the reference, per million (every 16th piece)   */
    uint64_t n_whole_tile_items;                  /* tiles piled up AND gated by one workgroup (sparse cohorts) */
    uint64_t n_listed_tiles;                      /* ... of which the last pass sent through the ordinary gate kernel: more candidate
                                                     positions than a tile's record list holds                                      */
} msnv_dataset_info;

int  msnv_dataset_info_get(const msnv_dataset *ds, msnv_dataset_info *out);
/* Cost of the per-read stage on the device for this dataset so far (csrc/devpack.hip), cumulative over its rounds:
 * out[0..4] kernel ms (HIP events on the context's stream) of record scan (the quick route, round 6: record boundaries AND the per-record measure,
 * one walk), per-record measure (careful route only), depth, emit (headers + bases + flags), tile-order sort; [5..7] wall seconds of uploading host streams, downloading headers / intervals, the host pre-pass (depth cap,
 * overlapping mates, token limit); [8] record bytes resident in HBM, [9] records, [10] pieces, [11] samples that took the pre-pass,
 * [12] scan segments whose guessed entry point was wrong and that were walked again, [13] deep (sample, tile) runs dealt into groups by
 * the device form of finalize, [14] samples whose dense block streams (short reads) were laid out by it, [15] rounds the quick route had
 * launched and the careful route took over (a sample that needs the sequential edits, more far-reaching reads than the list holds), [16] samples
 * whose depth cap / token limit ran as kernels (round 6; [11] counts the ones the host pre-pass still takes: MSNV_PREPASS=host, a template with
 * more alignments than the overlap kernel's slots, far-reaching reads), [17] 1 when finalize adopted a single round's column buffer as the
 * dataset's columns instead of copying it (devpack_place_columns; MSNV_NO_ADOPT=1 copies), [18] blocks of 64 records that msnv_emit_block
 * handed to msnv_emit_block_slow (every block under MSNV_EMIT=slow). */
#define MSNV_PACK_STATS 19
int  msnv_dataset_pack_stats(const msnv_dataset *ds, double *out, int32_t n);
/* Inspection hook: the bytes of one device column / index table of a finalized dataset ("hdr", "hdr4", "hdr8m", "blk", "seq", "qual",
 * "s_read_base", "s_seq_base", "ref4", "pairs", "work", "chunks", "cov_iv", "cov_pairs", "cov_work"; the other tables of the tile index:
 * "ref_lc", "tile_vbeg", "tile_vend", "tile_nslots", "active_tiles", "gather_tiles", "tile_slot_start", "tile_slot_u16", "tile_slot_wide",
 * "slot_off", "gate_tiles", "gate_tiles_dense", "gate_tiles_staged", "tile_stage_idx", "merged_groups", "tile_pair_start",
 * "tile_pair_merged", "s_cov_base", "tile_len", "tile_contig_dev"; a table the dataset's layout does not allocate holds 0 bytes).
 * out = NULL: size query.  The tests
 * use it to show that the device pack (csrc/devpack.hip) and the host pack (csrc/pack.cpp) build the same dataset byte for byte. */
int  msnv_dataset_fetch_column(msnv_dataset *ds, const char *name, uint8_t *out, uint64_t capacity, uint64_t *n_bytes);

typedef struct {
    float    ms_total;           /* all kernels of one pass, HIP events on the launch stream */
    float    ms_pileup;          /* the dominant kernel (msnv_pileup_tiles)                  */
    float    ms_gate, ms_gather, ms_decide, ms_coverage;   /* the tail split is recorded only with MSNV_PHASE_TIMES=1 (event records cost stream time) */
    uint64_t n_sites;            /* candidate positions that reached the decision kernel     */
    uint64_t n_called_pop, n_called_indiv;   /* output lines (before the first-line drop)    */
    uint64_t n_events, n_overflow;
    uint64_t algorithmic_bytes;  /* bytes the pileup kernel must read  */
} msnv_run_stats;

/* One pass of the hot path over the resident dataset: per-position / per-sample allele
 * histogram, calling rule, per-sample gather.  Results stay on the device until
 * msnv_write_calls / msnv_results_*.  Safe to call repeatedly (bench.py). */
int  msnv_pileup_run(msnv_dataset *ds, msnv_run_stats *stats);

/* Per-sample genome coverage (qaCompute arithmetic) over the resident dataset. */
/* n passes enqueued back to back with ONE host synchronisation at the end (stats: n entries, may be NULL): how a queue of
 * shards keeps the GPU busy -- the host round trip of msnv_pileup_run costs ~40 us of idle GPU per pass.  With overlap != 0
 * consecutive passes alternate between two HIP streams and two sets of intermediates, so the small tail kernels of one
 * pass run under the pileup kernel of the next (+5 % passes/s; per-kernel times are then those of kernels sharing the
 * chip).  The results are those of the last pass.  msnv_pileup_run must have run once before (it sizes the buffers). */
int  msnv_pileup_run_many(msnv_dataset *ds, int32_t n, int32_t overlap, msnv_run_stats *stats);
/* The HIP events and the pinned counter blocks a batch of n passes needs, created now (the first msnv_pileup_run_many call of that size
 * otherwise creates them inside its own time: ~0.5-1 ms of host work in front of the first pass). */
int  msnv_pileup_reserve(msnv_dataset *ds, int32_t n);
int  msnv_coverage_run(msnv_dataset *ds, msnv_run_stats *stats);
/* Both passes over the same resident columns (BASELINE configs[2]: qaCompute + snpCall fused on the device):
 * replaces running `qaCompute` per BAM (metaSNV.py:63-65) and then `samtools mpileup | snpCall` (:160-176) on
 * the same files.  Either stats pointer may be NULL. */
int  msnv_fused_run(msnv_dataset *ds, msnv_run_stats *pileup_stats, msnv_run_stats *coverage_stats);
/* Writes OUT / OUT.detail for sample `sample_idx` from the last msnv_coverage_run. */
int  msnv_write_coverage(msnv_dataset *ds, int32_t sample_idx, const char *cov_path, const char *detail_path);

/* ------------------------------------------------------------------------------------
 * qaCompute's -m, -p W and -x FILE from the resident dataset (csrc/covext_k.hip): the median of the per-position depth, the window
 * profile and the mean depth of named regions, for every sample in one pass over the coverage index -- replaces one single-threaded
 * `qaCompute -m -p W -x FILE` per BAM (qaCompute.cpp:100-123,173-190,215).  Runs after msnv_dataset_finalize, before or after
 * msnv_coverage_run; asking for none of the three launches nothing.  Regions are (header contig index, start, end), both ends inclusive,
 * in the index space of qaCompute.cpp:114-116 (index = 1-based position); a region with start > end or end >= contig length is
 * MSNV_EDOMAIN (the reference reads past its prefix sums there).
 * ------------------------------------------------------------------------------------ */
typedef struct {
    int32_t        want_median;     /* -m                                                   */
    int32_t        window;          /* -p W; 0 = no profile                                 */
    uint32_t       n_regions;       /* -x: entries of the three arrays below; 0 = none      */
    uint32_t       reserved;
    const int32_t *region_contig;
    const int32_t *region_start;
    const int32_t *region_end;
} msnv_cov_extras;
int  msnv_coverage_extras_run(msnv_dataset *ds, const msnv_cov_extras *what);
/* Results of the last msnv_coverage_extras_run.
 *   medians      int32[n_samples][n_contigs]: data[L / 2] of the depths sorted as radix.h sorts them (unsigned: a negative depth, which only a contig's
 *                last position can hold, orders last); 0 where the sample has no coverage on the contig; all 0 without want_median.
 *   window sums  of ONE sample, uint64, contig-major in header order: contig c holds (L - 1) / W windows of the loop of
 *                qaCompute.cpp:175-182 (window 0 = indices 0 .. W, window k = k W + 1 .. (k + 1) W) plus, when (L - 1) % W != 0, the
 *                trailing one of :183-185; none for L == 1.  A sum is taken modulo 2^64 like the reference's wSum.
 *                msnv_coverage_window_count gives the number of entries (0 without a window).
 *   region sums  uint64[n_samples][n_regions], the sum of the depth over [start, end].
 * msnv_coverage_extras_launches: kernel launches the run took (0 when nothing was asked for; at most 3 per batch of rows). */
int  msnv_coverage_medians(msnv_dataset *ds, int32_t *out, uint64_t capacity);
int  msnv_coverage_window_count(const msnv_dataset *ds, uint64_t *n_windows);
int  msnv_coverage_window_sums(msnv_dataset *ds, int32_t sample_idx, uint64_t *out, uint64_t capacity);
int  msnv_coverage_region_sums(msnv_dataset *ds, uint64_t *out, uint64_t capacity);
int  msnv_coverage_extras_launches(const msnv_dataset *ds, uint32_t *n_launches);
/* One line of a -x file (qaCompute.cpp:344): contig name (need not be in the header), start, end, alias. */
typedef struct { const char *contig; int32_t start, end; const char *alias; } msnv_cov_region;
/* msnv_write_coverage plus the files of the last msnv_coverage_extras_run: OUT takes the Median_Cov column (qaCompute.cpp:215,237,437)
 * when that run computed medians; profile_path (NULL: not written) is OUT.profile (:173-186,249-260), specific_path (NULL: not
 * written) OUT.specific (:100-123,604-615) for the lines `regions` of the -x file -- those that name a header contig must be, in
 * order, the regions of the run.  DESIGN.md section 7 lists the one divergence (a contig whose reads are all filtered). */
int  msnv_write_coverage_ex(msnv_dataset *ds, int32_t sample_idx, const char *cov_path, const char *detail_path, const char *profile_path,
                            const char *specific_path, const msnv_cov_region *regions, uint32_t n_regions);
/* msnv_coverage with -m, -p W and -x FILE: the one-BAM form behind the msnv_qacompute drop-in.  A regions file whose field
 * count is no multiple of four, or with an interval outside its contig, is MSNV_EDOMAIN. */
typedef struct {
    const char *bam_path;
    int32_t     max_cov;            /* -c                                  */
    int32_t     min_mapq;           /* -q, default 1                       */
    const char *out_cov_path;       /* OUT                                 */
    const char *out_detail_path;    /* OUT.detail (-d)                     */
    int32_t     want_median;        /* -m                                  */
    int32_t     window;             /* -p W; 0 = no OUT.profile            */
    const char *out_profile_path;   /* OUT.profile; needed when window > 0 */
    const char *regions_path;       /* -x FILE; NULL = no OUT.specific     */
    const char *out_specific_path;  /* OUT.specific; needed with -x        */
} msnv_cov_ex_args;
int  msnv_coverage_ex(msnv_ctx *ctx, const msnv_cov_ex_args *args);
/* ... over the reads that `qaCompute -a` keeps (the subsampler below: word from msnv_subsample_seed_word, frac of -a's argument); frac <= 0:
 * msnv_coverage_ex, or msnv_coverage when none of -m -p -x is asked for. */
int  msnv_coverage_sub(msnv_ctx *ctx, const msnv_cov_ex_args *args, uint32_t word, double frac);

/* Formats the last run as called_SNPs / indiv_called (call_vC.cpp:641-667).
 * ann_path / fasta_path feed the codon annotation (call_vC.cpp:604-633) and may be NULL. */
int  msnv_write_calls(msnv_dataset *ds, const char *called_path, const char *indiv_path,
                      const char *ann_path, const char *fasta_path);

/* Raw results of the last run (for tests and for the multi-GPU gather).
 * A site record is fixed width:  msnv_site header + n_samples x msnv_site_sample. */
typedef struct {
    int32_t  tid;        /* BAM-header contig index              */
    int32_t  pos;        /* 0-based position                     */
    uint32_t cov;        /* total coverage over all samples      */
    uint32_t n[4];       /* total A, C, G, T                     */
    uint8_t  pop_mask;   /* bit i: allele i (A,C,G,T) is a population SNV */
    uint8_t  ind_mask;   /* bit i: allele i is an individual SNV          */
    uint8_t  refchar;    /* FASTA character                      */
    uint8_t  dropped;    /* 1 = this is the first pileup line (call_vC.cpp:423) */
} msnv_site;

typedef struct { uint16_t cov; uint16_t n[4]; } msnv_site_sample;

/* Gene / codon annotation of one site (snpCall -g, call_vC.cpp:567-574,604-633), computed on the device.
 * gene = index of the annotation row (file order, rows with start > end excluded) or -1.
 * codon[x] for allele x (A,C,G,T): {flags, len_old | len_new << 4, old[3], new[3]}. */
#define MSNV_ANN_VALID      1
#define MSNV_ANN_CIRCULAR   2   /* gene with start == end: the reference drops the allele */
#define MSNV_ANN_SYNONYMOUS 4
typedef struct { int32_t gene; uint8_t codon[4][8]; } msnv_site_ann;

/* ------------------------------------------------------------------------------------
 * Multi-GPU form of the two invocations above (the reference's counterpart is its pool of
 * processes, metaSNV.py:55-78,196-215, where every split process inflates every BAM in full).  The BAMs are dealt to the
 * ranks for decoding -- every file is inflated exactly once in the whole job -- each decoder deals the records to the
 * rank that owns their contig (msnv_records_partition; the exchange is an all-to-all over RCCL, metasnv_amd/parallel.py),
 * every rank runs the kernels over its contigs, and rank 0 receives the small tables: site records (msnv_results_fetch ->
 * msnv_write_calls_records) and coverage accumulators (msnv_coverage_fetch -> msnv_write_coverage_records).
 * ------------------------------------------------------------------------------------ */
/* qaCompute's read bookkeeping for the "Other" block of OUT (qaCompute.cpp:461-473,518-526,642-654). */
typedef struct { uint32_t total_reads, unmapped, zero_quality, proper_pairs, duplicates, any_mapped; } msnv_sample_stats;
#define MSNV_COV_WORDS 17   /* per (sample, contig): covSum, hist[0..15] (qaCompute.cpp:142-165) */

/* Deals one sample's raw record stream to n_parts parts: a mapped record goes to part contig_owner[tid] (-1 = nobody),
 * order preserved; unmapped records are counted and dropped.  out: n_bytes bytes, receives the parts back to back;
 * part_bytes[n_parts] their sizes; stats (may be NULL) the sample's qaCompute statistics over ALL records. */
int  msnv_records_partition(const uint8_t *records, uint64_t n_bytes, const int32_t *contig_owner, int32_t n_contigs,
                            int32_t n_parts, int32_t cov_min_mapq, uint8_t *out, uint64_t *part_bytes, msnv_sample_stats *stats);
/* msnv_records_partition for n streams at once, ON THE DEVICE (csrc/devdeal.hip): the streams (host memory, or device memory when on_device
 * != 0) are dealt by kernels into `out` -- DEVICE memory of `capacity` bytes, e.g. the send tensor of an all-to-all over RCCL -- destination-
 * major: part 0 of stream 0, of stream 1, ..., part 1 of stream 0, ..., with `gap` bytes left free in front of every part (the caller's size
 * table; capacity >= sum of n_bytes + n_parts * gap).  part_bytes[i * n_parts + k] = bytes of stream i in part k; stats[i] = stream i's
 * qaCompute statistics; contig_bases (may be NULL; n_contigs entries, not cleared) += aligned bases per contig (msnv_records_contig_bases). */
/* ... for BAM FILES: their BGZF blocks are inflated and CRC-checked on the device and the record streams dealt from there (no host copy of the
 * inflated bytes); the headers are checked against the dataset's contigs.  record_bytes[i] = bytes of file i's record stream.  The files of a
 * call must fit ONE batch of the device inflate (1 GB of BAM; MSNV_EDOMAIN otherwise: the caller takes the host route). */
int  msnv_dataset_deal_bams_device(msnv_dataset *ds, const char *const *bam_paths, int32_t n, int32_t host_threads, const int32_t *contig_owner, int32_t n_parts,
                                   int32_t cov_min_mapq, uint8_t *out, uint64_t capacity, uint64_t gap, uint64_t *part_bytes, msnv_sample_stats *stats,
                                   uint64_t *record_bytes);
/* ... before the owners are known (the split planner holds decoded rounds): the files' record streams, inflated and checked on the device, are
 * left in `out` (DEVICE memory) -- stream i at out + rec_off[i], rec_bytes[i] long, 16 readable bytes behind it -- with their statistics and the
 * aligned bases per contig (contig_bases, n_contigs of the dataset, not cleared); msnv_records_deal_device (on_device != 0) deals them later. */
int  msnv_dataset_inflate_bams_device(msnv_dataset *ds, const char *const *bam_paths, int32_t n, int32_t host_threads, uint8_t *out, uint64_t capacity,
                                      uint64_t *rec_off, uint64_t *rec_bytes, msnv_sample_stats *stats, uint64_t *contig_bases);
/* A second context OF THE SAME DEVICE for the two calls above (NULL: back to the dataset's own): its stream, staging buffers and pinned
 * words carry the upload, inflate, CRC check and dealing of round k + 1 of the N-rank feed while the dataset's own context packs round k
 * (one thread per context) -- the reference overlaps its splits as concurrent processes, each of which reads every BAM
 * (/root/reference/metaSNV.py:196-215); here a round's files are read once, by the feed.  Nothing of the dataset is written through it. */
int  msnv_dataset_set_feed_ctx(msnv_dataset *ds, msnv_ctx *ctx);
int  msnv_records_deal_device(msnv_ctx *ctx, const uint8_t *const *streams, const uint64_t *n_bytes, int32_t n, int32_t on_device, const int32_t *contig_owner,
                              int32_t n_contigs, int32_t n_parts, int32_t cov_min_mapq, uint8_t *out, uint64_t capacity, uint64_t gap, uint64_t *part_bytes,
                              msnv_sample_stats *stats, uint64_t *contig_bases);
/* Adds the aligned (M/=/X) bases of every mapped record of a raw record stream to bases[tid] (n_contigs entries, not cleared):
 * the weight of the reference's split rule, genome length x coverage = aligned bases (src/createOptimumSplit.py:46-50), which
 * the N-rank driver takes from its first round of decoded BAMs before it fixes the contig owners. */
int  msnv_records_contig_bases(const uint8_t *records, uint64_t n_bytes, int32_t n_contigs, uint64_t *bases);

/* ------------------------------------------------------------------------------------
 * Reads subsampled by the hash of their name: `qaCompute -a SEED.FRAC` (qaCompute.cpp:319-325, :454-458), the rule of
 * `samtools view -s`.  A read is kept iff (wang(x31(name) ^ word) & 0xffffff) < ceil(frac * 2^24); mates share a name and so a
 * fate; a dropped read exists nowhere behind this stage (no statistic, no coverage, no pileup); the kept ones keep order and bytes.
 * x31 / wang are khash.h's string and integer hashes as restated in csrc/devsub.h (unpinned against a real qaCompute: DESIGN.md
 * section 7).  The name is the record's read_name up to its first NUL, at most l_read_name bytes.
 * frac <= 0 everywhere below means NO subsampling: nothing is launched, read or copied; frac >= 1 keeps every read.
 * ------------------------------------------------------------------------------------ */
/* word = 0 for seed 0, else libc's srand(seed); rand() (1 -> 1804289383 with glibc).  seed < 0 or > 4294967295: MSNV_EINVAL (the
 * reference truncates such a seed). */
int  msnv_subsample_seed_word(int64_t seed, uint32_t *word);
/* The rule for ONE name (NUL-terminated): 1 = kept, 0 = dropped (no error code; NULL is dropped).  frac <= 0 drops every name here --
 * the callers below never ask then. */
int  msnv_subsample_keep(const char *name, uint32_t word, double frac);
/* One stream on a host thread: the kept records to out (room for n_bytes bytes), *out_bytes of them; counts = {kept, dropped}.
 * frac <= 0: out is not touched, *out_bytes = n_bytes, counts = {0, 0}.  A malformed chain of records is MSNV_EFORMAT. */
int  msnv_records_subsample(const uint8_t *records, uint64_t n_bytes, uint32_t word, double frac, uint8_t *out, uint64_t *out_bytes, uint64_t counts[2]);
/* n streams (n <= 2048; host memory, or device memory when on_device != 0) ON THE DEVICE (csrc/devsub.hip): the kept records of stream i
 * go to out + out_off[i], out_bytes[i] of them; counts[2 * i] = kept, counts[2 * i + 1] = dropped.  out: DEVICE memory of `capacity`
 * bytes; stream i is given ((n_bytes[i] + 31) & ~15) bytes of it, whatever is kept -- it starts on 16 bytes and at least 16 readable bytes
 * lie behind it -- and a capacity below the sum of these is MSNV_EINVAL before anything is launched.  ms_kernel (may be NULL): kernel
 * milliseconds of the record scan and the stage.  frac <= 0: out is not touched, out_off[i] = UINT64_MAX (the stream is its own output),
 * out_bytes[i] = n_bytes[i], counts 0, *ms_kernel = 0.  A malformed chain of records is MSNV_EFORMAT. */
int  msnv_records_subsample_device(msnv_ctx *ctx, const uint8_t *const *streams, const uint64_t *n_bytes, int32_t n, int32_t on_device, uint32_t word, double frac,
                                   uint8_t *out, uint64_t capacity, uint64_t *out_off, uint64_t *out_bytes, uint64_t *counts, double *ms_kernel);
/* Every stream handed to the dataset from now on passes through the subsampler before it is packed: msnv_dataset_add_sample_records[_many],
 * msnv_dataset_add_sample_bam[s], msnv_dataset_add_sample_records_device, the staged and the synthetic samples -- on the device, into a buffer
 * of the round's own, unless the dataset packs on host threads (MSNV_PACK=host, no context).  msnv_dataset_sample_stats counts the kept reads.
 * Set BEFORE the first sample is added (later: MSNV_EINVAL); frac <= 0 switches it off.  While it is set,
 * msnv_dataset_add_sample_records_resident, msnv_dataset_deal_bams_device and msnv_dataset_inflate_bams_device refuse with MSNV_EINVAL and
 * leave the dataset as it was. */
int  msnv_dataset_set_subsample(msnv_dataset *ds, uint32_t word, double frac);
/* Statistics of sample `sample_idx` as counted while it was packed (only over the records this dataset was given). */
int  msnv_dataset_sample_stats(const msnv_dataset *ds, int32_t sample_idx, msnv_sample_stats *out);
/* Accumulators of the last msnv_coverage_run: acc[n_samples][n_contigs][MSNV_COV_WORDS], zeros for contigs outside the shard. */
int  msnv_coverage_fetch(msnv_dataset *ds, uint64_t *acc, uint64_t capacity_words);
/* The same accumulators as ROWS: one per (sample, contig) that has reads passing qaCompute's filter on this rank, in (sample, contig)
 * order -- what the device keeps and what a rank ships to rank 0.  The dense table above is n_samples x n_contigs x 136 bytes whatever
 * it holds (500 BAMs over a database of a million contigs: 68 GB); qaCompute itself prints a row per header contig per BAM
 * (qaCompute.cpp:226-263 for the ones without reads), which the writers below still do. */
int  msnv_coverage_rows_count(const msnv_dataset *ds, uint64_t *n_rows);
int  msnv_coverage_fetch_rows(msnv_dataset *ds, uint32_t *sample, uint32_t *contig, uint64_t *acc, uint64_t capacity_rows);
/* Writes OUT / OUT.detail of one sample from gathered accumulators acc[n_contigs][MSNV_COV_WORDS] exactly as
 * msnv_write_coverage does (qaCompute.cpp:192-217,226-263,439,623-657). */
int  msnv_write_coverage_records(const msnv_ref_desc *ref, int32_t max_cov, const msnv_sample_stats *stats, const uint64_t *acc,
                                 const char *cov_path, const char *detail_path);

/* First pileup line of this dataset's invocation (the one call_vC.cpp:423 drops); tid = -1 if no read passes. */
int  msnv_dataset_first_line(const msnv_dataset *ds, int32_t *tid, int32_t *pos);
/* Per contig (n = header contigs): position of the first pileup line of an invocation that starts at that contig, -1 when
 * no read of this dataset piles up there -- without -l (first_any) and under metaSNV's split BED `name 1 LEN`, which
 * excludes position 0 (first_from1; metaSNV.py:92).  Lets a driver that holds ONE resident dataset write every
 * best_split_K output with the first line that split's own snpCall process would have dropped (call_vC.cpp:423).
 * Only valid for datasets created without a BED restriction. */
int  msnv_dataset_first_lines(const msnv_dataset *ds, int32_t *first_any, int32_t *first_from1, int32_t n);
/* Formats site records that did not come from a local run (multi-GPU: records gathered from the
 * ranks over RCCL) exactly as msnv_write_calls does.  Records must be in (tid, pos) order. */
int  msnv_write_calls_records(const msnv_ref_desc *ref, int32_t n_samples, const msnv_site *sites,
                              const msnv_site_sample *samples, uint64_t n_sites,
                              const char *called_path, const char *indiv_path,
                              const char *ann_path, const char *fasta_path, const msnv_site_ann *ann);

/* Runs the annotation kernel over the sites of the last msnv_pileup_run.  The gene table and the codon genome are
 * parsed and uploaded on the first call for a given (ann_path, fasta_path) and stay resident; ms_kernel may be NULL. */
int  msnv_annotate_run(msnv_dataset *ds, const char *ann_path, const char *fasta_path, double *ms_kernel);
/* ann[n_sites] in the order of msnv_results_fetch. */
int  msnv_results_fetch_ann(msnv_dataset *ds, msnv_site_ann *ann, uint64_t capacity);

int  msnv_results_count(const msnv_dataset *ds, uint64_t *n_sites);
/* sites[n_sites], samples[n_sites * n_samples], both in (tid, pos) order. */
int  msnv_results_fetch(msnv_dataset *ds, msnv_site *sites, msnv_site_sample *samples, uint64_t capacity);
/* The same records with the per-sample part as ROWS OF CELLS (CSR) instead of n_samples entries per site: site i owns
 * cells [row_off[i], row_off[i + 1]) (row_off has n_sites + 1 entries), cell c belongs to sample cell_sample[c] (ascending
 * inside a row) and samples without a cell hold zeros.  This is what the device keeps (a cell per sample that has reads in the
 * site's tile) and what the ranks ship to rank 0: a 500-sample cohort whose species are each carried by a handful of samples
 * (BASELINE configs[3]) costs a handful of cells per site, where the dense form costs 5 KB.  The reference's counterpart is
 * the `c1|c2|...|cS` text of every called line (call_vC.cpp:316-325,635), S numbers whatever they are. */
int  msnv_results_cells_count(const msnv_dataset *ds, uint64_t *n_sites, uint64_t *n_cells);
int  msnv_results_fetch_cells(msnv_dataset *ds, msnv_site *sites, uint64_t *row_off, uint32_t *cell_sample, msnv_site_sample *cells,
                              uint64_t cap_sites, uint64_t cap_cells);
/* msnv_write_calls_records for records in the cell form (same text, byte for byte). */
int  msnv_write_calls_cells(const msnv_ref_desc *ref, int32_t n_samples, const msnv_site *sites, const uint64_t *row_off,
                            const uint32_t *cell_sample, const msnv_site_sample *cells, uint64_t n_sites,
                            const char *called_path, const char *indiv_path,
                            const char *ann_path, const char *fasta_path, const msnv_site_ann *ann);

/* ------------------------------------------------------------------------------------
 * Host I/O helpers used by the Python CLI and the tests (BGZF/BAM on zlib: htslib is not
 * available in the build image).
 * ------------------------------------------------------------------------------------ */
/* Host-stage counters since the library was loaded: BGZF blocks that the library's own DEFLATE decoder (csrc/inflate.cpp)
 * handed to zlib (0 for well-formed files; tests). */
int  msnv_host_stats(uint64_t *zlib_fallbacks);
/* Host-stage timers, cumulative seconds since the library was loaded or the last reset: [0] file reads, [1] host inflate + CRC checks,
 * [2] device inflate (wall: H2D, kernel, D2H), [3] parse + pack, [4] msnv_dataset_finalize (index build + upload, wall),
 * [5] text formatting of called_SNPs / indiv_called (wall), [6] msnv_dataset_add_sample_bams (wall).  [0], [1] and [3] are summed over
 * the host threads that did the work.  What the end-to-end block of bench.py splits a metaSNV.py run into; the reference's
 * counterpart is the wall time of its process pool (metaSNV.py:55-78,196-221). */
int  msnv_host_timers(double *seconds, int32_t n, int32_t reset);
/* The alignment-record streams of several BAM files in one call (the N-rank driver reads a round of files and deals their records to
 * the ranks that own the contigs: msnv_records_partition): through the device BGZF inflate when ctx is given and the files bring
 * >= 64 MB (MSNV_INFLATE overrides), else one host thread per file.  records[i], n_bytes[i]: the records behind the header of
 * bam_paths[i]; every records[i] is released with msnv_free.  Replaces the read loop `sam_read1` of qaCompute.cpp:441 / samtools. */
int  msnv_bam_records_many(msnv_ctx *ctx, const char *const *bam_paths, int32_t n, int32_t host_threads, uint8_t **records, uint64_t *n_bytes);
/* Test / measurement hook of the device BGZF inflate (csrc/inflate_k.hip): the inflated bytes of one BGZF
 * file, through the device (on_device != 0, needs ctx) or the host decoder.  *out is released with msnv_free.  counters (may be
 * NULL): [0] blocks, [1] blocks the device refused and the host inflated, [2] kernel microseconds, [3] inflated bytes. */
int  msnv_bgzf_inflate(msnv_ctx *ctx, const char *path, int32_t on_device, uint8_t **out, uint64_t *n_out, uint64_t counters[4]);
/* `samtools view -H` replacement for bed_header (metaSNV.py:81-94): writes SN\t1\tLN lines. */
int  msnv_bam_write_bed_header(const char *bam_path, const char *out_path);
/* Cores' worth of CPU time this process may use: the hardware threads, or the container's quota (cgroup cpu.max) when that is less. */
int32_t msnv_host_cores(void);
/* Reads a whole BAM: header text, contigs and the raw record stream.  Free with msnv_free. */
typedef struct {
    int32_t   n_contigs;
    char    **names;
    int64_t  *lengths;
    uint8_t  *records;
    uint64_t  n_record_bytes;
    char     *header_text;
} msnv_bam_data;
int  msnv_bam_read(const char *bam_path, msnv_bam_data *out);
/* ... the header alone (records = NULL): only the leading BGZF blocks are inflated (what `samtools view -H` reads, metaSNV.py:88). */
int  msnv_bam_read_header(const char *bam_path, msnv_bam_data *out);
void msnv_bam_data_free(msnv_bam_data *d);
/* Writes a BAM (BGZF) from a header and a raw record stream (synthetic inputs, tests). */
int  msnv_bam_write(const char *bam_path, const char *header_text, int32_t n_contigs,
                    const char *const *names, const int64_t *lengths,
                    const uint8_t *records, uint64_t n_record_bytes, int32_t compress_level);

/* ------------------------------------------------------------------------------------
 * Synthetic workload generator (SURVEY.md section 8d "testdata" shape).  Deterministic in
 * `seed`.  Produces the reference sequences and, per sample, a raw BAM record stream.
 * ------------------------------------------------------------------------------------ */
typedef struct {
    int32_t  n_species;          /* contigs refGenome{1..n}clus, one contig each            */
    int64_t  contig_len;
    int32_t  n_samples;
    int32_t  read_len;
    double   mean_cov;           /* per (sample, species): LogNormal(ln mean_cov, sigma)     */
    double   sigma_cov;
    double   frac_absent;        /* (sample, species) pairs with zero coverage               */
    double   snv_density;        /* subspecies SNV sites per position                        */
    double   error_rate;
    double   frac_lowq;          /* bases with BQ in [2,12]                                  */
    double   frac_indel_reads;   /* reads carrying one small I or D                          */
    double   frac_clip_reads;    /* reads with a leading soft/hard clip                      */
    double   frac_flagged;       /* DUP / SECONDARY / QCFAIL / mapq 0 reads (each)           */
    int32_t  lowercase_ref;      /* 1 = soft-mask 5 % of the reference (lower-case)           */
    uint64_t seed;
    double   frac_paired;        /* 0 (default, the BASELINE testdata shape is single-end): fraction of read starts that
                                    become a proper pair whose mates mostly overlap on the reference               */
    int32_t  contigs_per_species_max;   /* 0 / 1: one contig per species.  > 1 (BASELINE configs[2] / [3]): a species has
                                    1 .. max contigs `refGenome<k>clus.c<j>` that share contig_len bases           */
    int32_t  species_per_sample; /* 0: presence by frac_absent.  > 0: every sample draws that many random species and keeps
                                    each of them with probability 1 - frac_absent (fractional species counts of scaled shards) */
    double   frac_aux;           /* records that carry auxiliary fields behind the qualities, as every aligner writes them
                                    (NM:C, MD:Z, AS:i -- 18 bytes); 0 = none (the default workload's bytes do not change)       */
    double   frac_noseq;         /* records with SEQ `*` (l_seq = 0, CIGAR kept): in the pileup every base of such a read is N
                                    with quality 0; qaCompute counts its M blocks like any other                               */
} msnv_synth_params;

void msnv_synth_params_default(msnv_synth_params *p);
/* Number of contigs the parameters describe (= n_species unless contigs_per_species_max > 1). */
int  msnv_synth_contig_count(const msnv_synth_params *p);
/* Reference sequences: caller frees each seqs[i] and the arrays with msnv_free. */
int  msnv_synth_reference(const msnv_synth_params *p, char ***names, int64_t **lengths, char ***seqs);
/* One sample's raw BAM record stream (coordinate sorted). */
int  msnv_synth_sample(const msnv_synth_params *p, int32_t sample_idx, char *const *seqs,
                       uint8_t **records, uint64_t *n_bytes);
/* Generates samples [first, first+count) with a host thread pool and appends them to `ds`
 * (same bytes as msnv_synth_sample + msnv_dataset_add_sample_records, without the copies). */
int  msnv_dataset_add_synth_samples(msnv_dataset *ds, const msnv_synth_params *p, int32_t first, int32_t count,
                                    int32_t host_threads);
void msnv_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
