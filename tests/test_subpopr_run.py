"""metaSNV_subpopr.py's host half (metasnv_amd/subpopr_run.py) without a device: the argument forms, the output directory's name, rmNAfromDistMatrix
on hand-worked matrices, the front door's three result strings and the summaries against literal texts from small hand-written output trees."""
import os

import pytest

from metasnv_amd import core, subpopr, subpopr_run as run


class Quiet:
    def __init__(self):
        self.lines = []

    def say(self, msg=""):
        self.lines.append(msg)

    warn = say


# ---------------------------------------------------------------------------------------------- arguments
def test_logical_spellings(tmp_path):
    d = str(tmp_path)
    for text, value in (("TRUE", True), ("T", True), ("true", True), ("FALSE", False), ("F", False), ("false", False)):
        a = run.parse_args(["-i", d, "-m", text, "-r", text, "-q", text, "--useExistingClustering", text, "--useExistingGenotyping", text])
        assert (a.isMotus, a.createReports, a.onlyDoSubspeciesDetection, a.useExistingClustering, a.useExistingGenotyping) == (value,) * 5
    with pytest.raises(SystemExit):
        run.parse_args(["-i", d, "-q", "yes"])
    a = run.parse_args(["-i", d])                                          # the reference's defaults
    assert (a.outputDir, a.procs, a.sampleSuffix, a.speciesAbundance, a.geneAbundance, a.isMotus, a.createReports) == ("results", 1, "", "doNotRun", "doNotRun", True, True)
    assert (a.minNumSamples, a.fixReadThreshold, a.fixSnvThreshold, a.genotypingThreshold, a.clusterPSThreshold) == (100, 0.1, 0.8, 0.8, 0.8)
    assert (a.onlyDoSubspeciesDetection, a.useExistingClustering, a.useExistingGenotyping, a.seed, a.device, a.stability_iters, a.boot) == (False, False, False, None, 0, None, None)
    a = run.parse_args(["-i", d, "-p", "8", "--seed", "7", "--stability-iters", "2", "--boot", "5", "--minNumSamples", "12"])
    assert (a.procs, a.seed, a.stability_iters, a.boot, a.minNumSamples) == (8, 7, 2, 5, 12)


@pytest.mark.parametrize("flag,name", [("-x", "fixReadThreshold"), ("-y", "fixSnvThreshold"), ("-z", "genotypingThreshold"), ("--clusterPSThreshold", "clusterPSThreshold")])
@pytest.mark.parametrize("bad", ["1.5", "-0.1", "nan"])
def test_thresholds_outside_0_to_1_are_refused(tmp_path, flag, name, bad):
    with pytest.raises(SystemExit) as e:
        run.parse_args(["-i", str(tmp_path), flag + "=" + bad])
    assert str(e.value) == 'Param "' + name + '"must be numeric and must be between 0 and 1'      # assert0to1's message, its missing blank included
    assert os.listdir(str(tmp_path)) == []


def test_missing_inputs_are_refused_with_the_references_messages(tmp_path):
    with pytest.raises(SystemExit) as e:
        run.parse_args(["-o", str(tmp_path)])
    assert str(e.value) == "Path to metaSNV results must be supplied [-i]"
    for flag, kind in (("-a", "Species abundance"), ("-g", "Gene family abundance"), ("-i", "MetaSNV output directory")):
        missing = str(tmp_path / "nothing")
        with pytest.raises(SystemExit) as e:
            run.parse_args((["-i", str(tmp_path)] if flag != "-i" else []) + [flag, missing, "-m", "FALSE"])
        assert str(e.value) == kind + " file specified but does not exist: " + missing


def test_species_abundance_with_motus_is_refused_before_anything_is_created(tmp_path):
    proj = tmp_path / "proj"
    proj.mkdir()
    abund = tmp_path / "species.tsv"
    abund.write_text("\ts1\n101\t0.5\n")
    out = tmp_path / "results"
    for extra in ([], ["-m", "TRUE"]):
        with pytest.raises(SystemExit) as e:
            run.main(["-i", str(proj), "-o", str(out), "-a", str(abund)] + extra)
        assert "not built" in str(e.value) and "-m FALSE" in str(e.value)
    assert not out.exists()


def test_output_directory_name(tmp_path):
    d = str(tmp_path / "proj")
    name = lambda *argv: run.out_dir_of(run.parse_args(["-i", d + "/", "-o", "res"] + list(argv)))
    os.makedirs(d)
    assert name() == os.path.join("res", "params.hr10.hs80.ps80.gs80", "proj")
    assert name("-x", "0.075") == os.path.join("res", "params.hr7.5.hs80.ps80.gs80", "proj")
    assert name("-x", "0.29", "-y", "0.5", "-z", "1", "--clusterPSThreshold", "0") == os.path.join("res", "params.hr29.hs50.ps0.gs100", "proj")
    assert 0.29 * 100 != 29.0                                             # the product is printed with 15 digits, as R pastes it


@pytest.mark.skipif(core.device_count() > 0, reason="GPU present: the no-device failure path is not reachable")
def test_driver_refuses_to_run_without_a_gpu(tmp_path):
    proj = tmp_path / "proj"
    proj.mkdir()
    with pytest.raises(SystemExit) as e:
        run.main(["-i", str(proj), "-o", str(tmp_path / "results")])
    assert "no CPU fallback" in str(e.value)
    assert not (tmp_path / "results").exists()


# ---------------------------------------------------------------------------------------------- rmNAfromDistMatrix
def matrix(n, na_pairs=(), all_na=(), blank="NA"):
    cells = [["0" if i == j else "0.%d" % (1 + abs(i - j)) for j in range(n)] for i in range(n)]
    for i, j in na_pairs:
        cells[i][j] = cells[j][i] = blank
    for i in all_na:
        for j in range(n):
            cells[i][j] = cells[j][i] = blank
    return cells


def test_na_removal_on_hand_worked_matrices():
    assert run.rm_na_from_dist_matrix(matrix(3, all_na=[1])) == [0, 2]                       # a sample that is all NA, its diagonal included
    assert run.rm_na_from_dist_matrix(matrix(3, all_na=[1], blank="")) == [0, 2]              # ... written as empty cells
    assert run.rm_na_from_dist_matrix(matrix(3, na_pairs=[(0, 1)])) == [1, 2]                 # one NA pair: one NA each, the first in matrix order goes
    assert run.rm_na_from_dist_matrix(matrix(4, na_pairs=[(2, 3)], blank="")) == [0, 1, 3]
    # a chain: 1 has two NA cells, 0 and 2 one each; removing 1 clears both, so 0 and 2 stay
    assert run.rm_na_from_dist_matrix(matrix(4, na_pairs=[(0, 1), (1, 2)])) == [0, 2, 3]
    # two rounds: 0-1, 0-2, 3-4: 0 goes first (two NA cells), then 3 (tie with 4, first in matrix order)
    assert run.rm_na_from_dist_matrix(matrix(5, na_pairs=[(0, 1), (0, 2), (3, 4)])) == [1, 2, 4]
    assert run.rm_na_from_dist_matrix(matrix(4)) == [0, 1, 2, 3]
    assert run.rm_na_from_dist_matrix([]) == []


def write_project_tables(tmp_path, names, cells, freq_names):
    dist, freq = str(tmp_path / "sp.filtered.mann.dist"), str(tmp_path / "sp.filtered.freq")
    run.write_dist_text(dist, names, cells, list(range(len(names))))
    with open(freq, "w") as f:
        f.write("\t" + "\t".join(freq_names) + "\nc1:-:1:A:.\t" + "\t".join("0.5" for _ in freq_names) + "\n")
    return dist, freq


def test_a_table_without_na_is_handed_on_as_it_is(tmp_path):
    names = ["a.bam", "b.bam", "c.bam"]
    dist, freq = write_project_tables(tmp_path, names, matrix(3), names)
    out = str(tmp_path / "out")
    os.makedirs(out)
    assert run.clean_inputs("sp", dist, freq, out, 3, Quiet()) == (dist, None)
    assert os.listdir(out) == []                                          # no inputs/ directory


def test_a_cleaned_table_keeps_the_survivors_text(tmp_path):
    names = ["a.bam", "b.bam", "c.bam", "d.bam"]
    cells = matrix(4, na_pairs=[(0, 1), (1, 2)], blank="")
    cells[0][3] = cells[3][0] = "1.2500000000000001e-01"                  # not how any printer here would write it
    dist, freq = write_project_tables(tmp_path, names, cells, ["d.bam", "a.bam", "c.bam", "x.bam"])      # another order, b.bam missing, one more
    assert run.read_dist_text(dist) == (names, cells)
    out = str(tmp_path / "out")
    log = Quiet()
    path, reason = run.clean_inputs("sp", dist, freq, out, 3, log)
    assert reason is None and path == os.path.join(out, "inputs", "sp.filtered.mann.dist")
    assert open(path).read() == "\ta.bam\tc.bam\td.bam\na.bam\t0\t0.3\t1.2500000000000001e-01\nc.bam\t0.3\t0\t0.2\nd.bam\t1.2500000000000001e-01\t0.2\t0\n"
    assert any("Samples names do not match" in ln and "3 samples" in ln for ln in log.lines)


def test_result_strings_of_the_size_checks(tmp_path):
    names = ["a.bam", "b.bam", "c.bam"]
    out = str(tmp_path / "out")
    dist, freq = write_project_tables(tmp_path, names, matrix(3), ["a.bam", "b.bam"])
    assert run.clean_inputs("sp", dist, freq, out, 3, Quiet()) == (
        None, "Too few samples remain after selecting only those in the distance and SNP files. At least 3 are required for analysis.")
    dist, freq = write_project_tables(tmp_path, names, matrix(3), names)
    assert run.clean_inputs("sp", dist, freq, out, 100, Quiet()) == (None, "Insufficient number of samples in metaSNV filtered SNV results (3 samples)")
    dist, freq = write_project_tables(tmp_path, names, matrix(3, na_pairs=[(0, 1)]), names[1:])     # the count is the distance table's, after the NA rule
    assert run.clean_inputs("sp", dist, freq, out, 12, Quiet()) == (None, "Insufficient number of samples in metaSNV filtered SNV results (2 samples)")
    dist, freq = write_project_tables(tmp_path, names[:1], matrix(1), names[:1])                  # length(distMa) < 2
    assert run.clean_inputs("sp", dist, freq, out, 1, Quiet()) == (None, "Insufficient number of samples in metaSNV dist matrix results (1 samples)")
    assert not os.path.exists(out)


def test_species_are_those_with_both_tables_in_byte_order(tmp_path):
    os.makedirs(str(tmp_path / "distances"))
    os.makedirs(str(tmp_path / "filtered" / "pop"))
    for sp in ("505", "B2", "101", "a1"):
        (tmp_path / "distances" / (sp + ".filtered.mann.dist")).write_text("")
    (tmp_path / "distances" / "101.filtered.allele.dist").write_text("")
    for sp in ("a1", "101", "B2", "606"):
        (tmp_path / "filtered" / "pop" / (sp + ".filtered.freq")).write_text("")
    assert run.species_of(str(tmp_path)) == (["101", "B2", "a1"], ["505", "606"])
    assert run.species_of(str(tmp_path / "nothing")) == ([], [])


# ---------------------------------------------------------------------------------------------- the summaries
def output_tree(out):
    """Species 101 (two clusters, extended, two position files), 1 (a prefix of 101 and of 10; extended, one position file), 10 (two clusters, no
    extended clustering) and 202 (in noClustering/)."""
    os.makedirs(os.path.join(out, "noClustering"))
    put = lambda rel, text: open(os.path.join(out, rel), "w").write(text)
    put("noClustering/202_mann_clustering.tab", "clust\ns1\t1\ns2\t1\n")
    for sp in ("101", "1", "10"):
        put(sp + "_mann_clustering.tab", "clust\ns1\t1\ns2\t2\ns3\t1\n")
    put("101_extended_clustering.tab", "clust\ns1\t1\ns2\t2\ns3\t1\ns4\tNA\n")
    put("1_extended_clustering.tab", "clust\ns1\t2\ns2\t1\n")
    put("101_1_hap_positions.tab", "posId\tflip\np1\tFALSE\np2\tTRUE\np3\tFALSE\n")
    put("101_2_hap_positions.tab", "posId\tflip\np4\tFALSE\np5\tFALSE\n")
    put("1_1_hap_positions.tab", "posId\tflip\np9\tFALSE\n")
    put("101_extended_clustering_wFreq.tab", "1\t2\ns1\t100\t0\ns2\t0\t100\ns3\t60\t30\ns4\t100\t25\n")
    put("1_extended_clustering_wFreq.tab", "1\t2\ns1\t100\t0\ns2\t0\t100\n")
    put("101_clust_1_hap_coverage_extended_normed.tab", "X1\ns2\t0.5\ns1\t0.250\n")
    put("101_clust_2_hap_coverage_extended_normed.tab", "X2\ns1\t0\n")


def test_clustering_extension_summary(tmp_path):
    out = str(tmp_path)
    output_tree(out)
    assert run.clustered_species(out) == ["1", "10", "101", "202"]
    run.summarise_clustering_extension(out)
    # "1_.*_hap_positions.tab" is not anchored: it also finds 101's two files, which stand before 1_1 in byte order
    assert open(os.path.join(out, "summary_clusteringExtension.csv")).read() == (
        '"speciesID","ClusterGenotyping","GenotypedClusterSizes","nSNVs"\n'
        '"1","Succeeded","1-1","3-2-1"\n'
        '"10","Failed","NA","NA"\n'
        '"101","Succeeded","2-1","3-2"\n'
        '"202","No clusters","NA","NA"\n')


def test_subpop_completeness_summary(tmp_path):
    out = str(tmp_path)
    output_tree(out)
    run.assess_subpop_completeness(out)
    assert open(os.path.join(out, "subpopFreqSumsStats.tsv")).read() == (
        "species\tnClus\tnSamples\teq100\tgt100\tgt110\tgt120\tlt100\tlt90\tlt80\tlt50\twarningFlag\n"
        "101\t2\t4\t0.5\t0.25\t0.25\t0.25\t0.25\t0\t0\t0\tTRUE\n"
        "1\t2\t2\t1\t0\t0\t0\t0\t0\t0\t0\tFALSE\n")
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    assert run.assess_subpop_completeness(empty) == [] and os.listdir(empty) == []


def test_subpop_abundance_collection(tmp_path):
    out = str(tmp_path)
    output_tree(out)
    assert run.collect_subpop_abunds(out) == 3
    assert open(os.path.join(out, "subpopAbunds.tsv")).read() == "sampleName\tspecies\tsubpop\tabundance\ns1\t101\t1\t0.250\ns1\t101\t2\t0\ns2\t101\t1\t0.5\n"
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    assert run.collect_subpop_abunds(empty) is None and os.listdir(empty) == []


CLUSTERING_COLUMNS = ('"speciesID","speciesName","numberOfSamplesUsedForClusterDetection","numberOfClusters","predictionStrengthValue","confidenceInNumberOfClusters",'
                      '"confidencePerCluster","clusterSizes","detailedClusteringResultsFile"')


def test_all_results_summary(tmp_path):
    out = str(tmp_path)
    output_tree(out)
    subpopr.summarise_clustering(out)                                     # rows in the byte order of the files' paths: 101, 10, 1, 202
    assert run.combine_all_summaries(out) == 4                            # -q: from the clustering summary alone
    row = lambda sp, sub="": '"%s",NA,NA,1,NA,NA,NA,NA,"./%s%s_detailedSpeciesReport.html"' % (sp, sub, sp)
    assert open(os.path.join(out, "summary_allResults.csv")).read() == CLUSTERING_COLUMNS + "\n" + row("1") + "\n" + row("10") + "\n" + row("101") + "\n" \
        + row("202", "noClustering/") + "\n"
    run.summarise_clustering_extension(out)
    run.combine_all_summaries(out)
    assert open(os.path.join(out, "summary_allResults.csv")).read() == (
        CLUSTERING_COLUMNS + ',"ClusterGenotyping","GenotypedClusterSizes","nSNVs"\n'
        + row("1") + ',"Succeeded","1-1","3-2-1"\n'
        + row("10") + ',"Failed","NA","NA"\n'
        + row("101") + ',"Succeeded","2-1","3-2"\n'
        + row("202", "noClustering/") + ',"No clusters","NA","NA"\n')
    put = lambda rel, text: open(os.path.join(out, rel), "w").write(text)
    put("101_corrGenes-spearman.tsv", "gene\testimate\ng1\t0.9\n")
    put("101_corrGenes-pearson.tsv", "gene\testimate\n")
    put("1_corrGenes-spearman.tsv", "gene\testimate\ng1\t0.9\n")
    put("1_corrGenes-pearson.tsv", "gene\testimate\ng1\t0.9\n")
    put("1_corrGenes-clusterSpecificGenes.tsv", "gene\tcluster\ng1\t1\n")
    run.summarise_gene_family_correlations(out, "Genes")
    assert open(os.path.join(out, "summary_geneFamilyCorrAssoc.csv")).read() == (
        '"speciesID","geneFamCorrTested","anySignifGeneFamCorrs","detailedGeneFamCorrResultsFile"\n'
        '"1","Correlations calculated",TRUE,"./1_geneContentReport.html"\n'
        '"10","No correlation results",FALSE,NA\n'
        '"101","Only one correlation result file present",FALSE,"./101_geneContentReport.html"\n'
        '"202","No correlation results",FALSE,NA\n')
    run.combine_all_summaries(out)
    assert open(os.path.join(out, "summary_allResults.csv")).read().splitlines()[3] == (
        row("101") + ',"Succeeded","2-1","3-2","Only one correlation result file present",FALSE,"./101_geneContentReport.html"')


def test_results_per_species_file(tmp_path):
    run.write_results_per_species(str(tmp_path), {"101": "nClusters = 2", "202": 'ERROR: cell "x"'})
    assert open(str(tmp_path / "log_clusteringSummaryPerSpecies.txt")).read() == '"result" "species"\n"nClusters = 2" "101"\n"ERROR: cell \\"x\\"" "202"\n'
