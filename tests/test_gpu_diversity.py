"""metaSNV_DistDiv.py --div / --divNS / --matched on the device (msnv_div_file through metasnv_amd.distdiv): byte-identical
with the files the reference script wrote (tests/golden/python_callers/diversity), and with the test-side model
(tests/divmodel.py, itself pinned against those files by tests/test_diversity_model.py) on random tables.  In these tables a
pair's count of valid rows is whatever the seed gave; the counts at which the kernel's loops change shape are prescribed in
tests/divcases.py and run by tests/test_gpu_div_sizes.py."""
import json
import os
import random
import shutil

import pytest

import divmodel

pytestmark = pytest.mark.gpu


def _golden(golden_dir):
    return os.path.join(golden_dir, "python_callers", "diversity")


def _run(args):
    from metasnv_amd import distdiv
    distdiv.main(args)


@pytest.mark.parametrize("run", ["div_divNS", "div_matched", "dist_matched", "divNS_matched"])
def test_reference_files_byte_identical(tmp_path, golden_dir, run):
    g = _golden(golden_dir)
    spec = json.load(open(os.path.join(g, "runs.json")))[run]
    proj = str(tmp_path / "proj")                              # the table names derive from the directory name
    shutil.copytree(os.path.join(g, "proj"), proj)
    _run(["--filt", os.path.join(proj, "filtered-m5-d2", "pop"), "--n_threads", "4"] + spec["options"])
    assert sorted(d for d in os.listdir(proj) if d.startswith("distances")) == [spec["outdir"]]
    want_dir = os.path.join(g, "expected", run)
    got_dir = os.path.join(proj, spec["outdir"])
    assert sorted(os.listdir(got_dir)) == sorted(os.listdir(want_dir))
    for f in os.listdir(want_dir):
        assert open(os.path.join(got_dir, f)).read() == open(os.path.join(want_dir, f)).read(), (run, f)


def test_table_without_s_rows_fails_like_the_reference(tmp_path, golden_dir):
    g = _golden(golden_dir)
    assert json.load(open(os.path.join(g, "noS", "result.json")))["reference_fails"]
    proj = str(tmp_path / "proj")
    shutil.copytree(os.path.join(g, "noS", "proj"), proj)
    with pytest.raises(SystemExit) as e:
        _run(["--filt", os.path.join(proj, "filtered-m5-d2", "pop"), "--divNS"])
    assert e.value.code not in (None, 0)
    assert "synonymous (S)" in str(e.value) and "gene annotation" in str(e.value)


def test_unknown_species_or_sample_is_named(tmp_path, golden_dir):
    g = _golden(golden_dir)
    proj = str(tmp_path / "proj")
    shutil.copytree(os.path.join(g, "proj"), proj)
    pop = os.path.join(proj, "filtered-m5-d2", "pop")
    shutil.copy(os.path.join(pop, "spB.filtered.freq"), os.path.join(pop, "spQ.filtered.freq"))
    with pytest.raises(SystemExit) as e:
        _run(["--filt", pop, "--div"])
    assert "spQ" in str(e.value)
    os.remove(os.path.join(pop, "spQ.filtered.freq"))
    text = open(os.path.join(pop, "spB.filtered.freq")).read().replace("s3.bam", "sX.bam", 1)
    open(os.path.join(pop, "spB.filtered.freq"), "w").write(text)
    with pytest.raises(SystemExit) as e:
        _run(["--filt", pop, "--div"])
    assert "sX.bam" in str(e.value)


def _value(rnd, nan_rate):
    if rnd.random() < nan_rate:
        return "-1"
    c = rnd.choice([1, 2, 3, 7, 40, 97, 1000, 29989, 200003])
    return repr(rnd.randint(0, c) / c)


def _random_project(root, rnd, species):
    """species: {name: (n_samples, n_single, group sizes, nan rates)} -> the project directory."""
    proj = os.path.join(root, "rproj")
    pop = os.path.join(proj, "filtered", "pop")
    os.makedirs(pop)
    n_max = max(s[0] for s in species.values())
    samples = ["x%d.bam" % i for i in range(n_max)]
    cov = "\t" + "\t".join(samples) + "\nTaxId\t" + "\t".join(["Average_cov"] * n_max) + "\n"
    perc = "\t" + "\t".join(samples) + "\nTaxId\t" + "\t".join(["Percentage_1x"] * n_max) + "\n"
    bed = ""
    for sp, (S, n_single, groups, nan) in species.items():
        labels = []
        pos = iter(rnd.sample(range(1, 10 ** 6), n_single + len(groups)))
        tag = lambda: rnd.choice(["N[ATG-ACG]", "S[GCT-GCC]", "S[TA-TC]", "."])
        for k in range(n_single):
            t = "N[ATG-ACG]" if k == 0 else "S[GCT-GCC]" if k == 1 else tag()     # both classes present (--divNS)
            labels.append("%s.c%d:%s:%d:A>T:%s" % (sp, k % 3, rnd.choice(["-", "g1", "g22"]), next(pos), t))
        for m in groups:
            key = "%s.c%d:%s:%d" % (sp, rnd.randint(0, 2), rnd.choice(["-", "g1"]), next(pos))
            labels.extend("%s:%s>G:%s" % (key, "ACGT"[k % 4], tag()) for k in range(m))
        rnd.shuffle(labels)
        cols = samples[:S]
        with open(os.path.join(pop, "%s.filtered.freq" % sp), "w") as f:
            f.write("\t" + "\t".join(cols) + "\n")
            for l in labels:
                f.write(l + "\t" + "\t".join(_value(rnd, nan[s]) for s in range(S)) + "\n")
        cov += sp + "\t" + "\t".join("%f" % rnd.choice([0.0, 1.0, 1.5, 2.0, 7.25, 30.0]) for _ in samples) + "\n"
        perc += sp + "\t" + "\t".join("%f" % rnd.choice([0.0, 12.5, 50.0, 97.3, 100.0]) for _ in samples) + "\n"
        for c in range(3):
            bed += "%s.c%d\t1\t%d\n" % (sp, c, rnd.randint(100, 100000))
    open(os.path.join(proj, "rproj.all_cov.tab"), "w").write(cov)
    open(os.path.join(proj, "rproj.all_perc.tab"), "w").write(perc)
    open(os.path.join(proj, "bed_header"), "w").write(bed)
    return proj


def _check_against_model(proj, options):
    pop = os.path.join(proj, "filtered", "pop")
    _run(["--filt", pop] + options)
    outdir = os.path.join(proj, "distances.matched_pos" if "--matched" in options else "distances")
    want = divmodel.project_outputs(pop, options)
    assert sorted(os.listdir(outdir)) == sorted(want)
    for name, text in want.items():
        assert open(os.path.join(outdir, name)).read() == text, (options, name)
    shutil.rmtree(outdir)


def test_random_tables_against_the_model(tmp_path):
    """S up to 24, up to 20 000 rows, 2 000 multi-allelic positions with m up to 12, > 8 192 valid single rows per pair,
    NaN-heavy and all-NaN columns, an all-numeric species name (looked up by its text), tiny tables."""
    rnd = random.Random(17)
    big_groups = [rnd.choice([2, 2, 2, 2, 3, 3, 4]) for _ in range(1990)] + [5, 6, 7, 8, 9, 10, 11, 12, 12, 11]
    species = {
        "spBig": (24, 15500, big_groups, [0.01] * 20 + [0.7, 0.9, 1.0, 0.3]),
        "777": (5, 300, [2, 3, 12], [0.1, 0.5, 0.0, 0.2, 0.1]),
        "spTiny": (3, 4, [2], [0.0, 0.3, 0.3]),
        "spOne": (1, 20, [2, 2, 3], [0.2]),
        "spPair": (2, 200, [2, 3, 3], [0.1, 0.4]),
        "spNoGroup": (4, 1000, [], [0.05, 0.05, 0.5, 0.05]),
    }
    proj = _random_project(str(tmp_path), rnd, species)
    _check_against_model(proj, ["--div", "--divNS"])
    del species["spBig"]
    species["spMid"] = (12, 9000, [rnd.choice([2, 3, 4, 12]) for _ in range(300)], [0.02] * 10 + [0.15, 0.6])
    proj = _random_project(str(tmp_path / "m"), rnd, species)
    _check_against_model(proj, ["--div", "--divNS", "--matched"])


def test_random_table_of_70_samples_against_the_model(tmp_path):
    """msnv_div_pairs past 24 samples: 2 485 pairs through the triangle unranking and the i * n_samples + j stores.  Few rows,
    so that the model (one pair at a time) stays affordable; an all-NaN and two NaN-heavy samples, groups up to m = 12."""
    rnd = random.Random(70)
    species = {"spWide": (70, 260, [2] * 14 + [3] * 6 + [4, 5, 12], [0.05] * 66 + [0.7, 1.0, 0.02, 0.5])}
    proj = _random_project(str(tmp_path), rnd, species)
    assert len(open(os.path.join(proj, "filtered", "pop", "spWide.filtered.freq")).readline().split("\t")) == 71
    _check_against_model(proj, ["--div", "--divNS"])
    _check_against_model(proj, ["--div", "--matched"])
