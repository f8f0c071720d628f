#!/usr/bin/env python
"""Generates tests/golden/python_callers/diversity/* by RUNNING the reference's metaSNV_DistDiv.py (--div, --divNS,
--matched, --dist) from /root/reference on synthetic projects.  Only inputs and outputs are kept (data, not source).
Re-run in the build container:  python tests/golden/make_diversity_goldens.py

  proj/                    the inputs: filtered-m5-d2/pop/{spA,spB,spC}.filtered.freq, proj.all_{cov,perc}.tab, bed_header
  expected/<run>/          what the reference wrote into distances<pars>[.matched_pos]/ for one option set (runs.json)
  noS/                     a project whose species has no S row; result.json records that the reference fails on --divNS

spA (7 samples): > 1 100 valid single rows per pair, > 128 multi-allelic positions with m = 2, 3, 4, one with m = 10 and
one with m = 12 (outer products beyond numpy's 8192-element block), 17 tied rows of one key (numpy's quicksort permutes
them), positions whose string order is not their numeric order, an all-NaN sample, a NaN-heavy one, Average_cov 1.0 and
0.0 and a Percentage_1x of 0 (inf, -0.0 and nan in the outputs).  spB: 2 samples (the --matched quirk).  spC: contigs
with several dotted names in bed_header.
"""
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "python_callers", "diversity")
PARS = "filtered-m5-d2"
RUNS = {"div_divNS": ["--div", "--divNS"], "div_matched": ["--div", "--matched"], "dist_matched": ["--dist", "--matched"],
        "divNS_matched": ["--divNS", "--matched"]}
SAMPLES = ["s%d.bam" % i for i in range(7)]
DENOMS = [2, 3, 4, 5, 7, 8, 10, 16, 20, 40, 97]


def w(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def value(rnd, nan_rate):
    if rnd.random() < nan_rate:
        return "-1"
    c = rnd.choice(DENOMS)
    return repr(rnd.randint(0, c) / c)


def table(rnd, samples, contigs, n_single, group_sizes, nan_rates, tied=0):
    """Rows of one species table, shuffled: single positions, multi-allelic ones (m rows with one key), one key of `tied` rows."""
    rows = []
    pos = iter(rnd.sample(range(1, 100000), n_single + len(group_sizes) + 1))
    syn = ["N[ATG-ACG]", "S[GCT-GCC]", "."]

    def label(ctg, gene, p, k):
        return "%s:%s:%d:%s:%s" % (ctg, gene, p, "ACGT"[k % 4] + ">" + "ACGT"[(k + 1) % 4], rnd.choice(syn))

    for k in range(n_single):
        rows.append(label(rnd.choice(contigs), rnd.choice(["-", "g%d" % k]), next(pos), k))
    for m in group_sizes + ([tied] if tied else []):
        ctg, gene, p = rnd.choice(contigs), rnd.choice(["-", "gm"]), next(pos)
        rows.extend(label(ctg, gene, p, k) for k in range(m))
    rnd.shuffle(rows)
    text = "\t" + "\t".join(samples) + "\n"
    for r in rows:
        text += r + "\t" + "\t".join(value(rnd, nan_rates[s]) for s in range(len(samples))) + "\n"
    return text


def make_project(proj):
    rnd = random.Random(2024)
    pop = os.path.join(proj, PARS, "pop")
    # spA: 9 and 10, 99 and 100 ... land in string order; s4 all NaN, s5 NaN-heavy
    w(os.path.join(pop, "spA.filtered.freq"),
      table(rnd, SAMPLES, ["spA.c1", "spA.c2"], 1400, [2] * 120 + [3] * 50 + [4] * 27 + [10, 12], [.03, .03, .03, .03, 1.0, .6, .03], tied=17))
    w(os.path.join(pop, "spB.filtered.freq"), table(rnd, ["s0.bam", "s3.bam"], ["spB.q"], 60, [2] * 8 + [3] * 3, [.1, .3]))
    w(os.path.join(pop, "spC.filtered.freq"), table(rnd, ["s1.bam", "s2.bam", "s5.bam", "s6.bam"], ["spC.x.c1", "spC.y.c2", "spC.z"], 150,
                                                   [2] * 20 + [3] * 5, [.1, .1, .2, .05]))
    cov = {"spA": [1.0, 0.0, 7.25, 12.0, 3.5, 9.125, 2.0], "spB": [5.5, 2.0, 2.0, 30.0, 2.0, 2.0, 2.0], "spC": [2.0, 8.0, 3.0, 1.5, 2.0, 44.0, 6.0]}
    perc = {"spA": [80.0, 55.5, 0.0, 99.0, 41.0, 12.5, 63.0], "spB": [50.0, 50.0, 50.0, 75.25, 50.0, 50.0, 50.0],
            "spC": [10.0, 90.0, 33.3, 70.0, 5.0, 66.0, 20.0]}
    for name, head, vals in (("proj.all_cov.tab", "Average_cov", cov), ("proj.all_perc.tab", "Percentage_1x", perc)):
        text = "\t" + "\t".join(SAMPLES) + "\nTaxId\t" + "\t".join([head] * len(SAMPLES)) + "\n"
        for sp in sorted(vals):
            text += sp + "\t" + "\t".join("%f" % x for x in vals[sp]) + "\n"
        w(os.path.join(proj, name), text)
    w(os.path.join(proj, "bed_header"), "spA.c1\t1\t5000\nspA.c2\t1\t2500\nspB.q\t1\t900\nspC.x.c1\t1\t1200\nspC.y.c2\t1\t800\nspC.z\t1\t333\n")


def run_reference(proj, options):
    return subprocess.run([sys.executable, os.path.join(REF, "metaSNV_DistDiv.py"), "--filt", os.path.join(proj, PARS, "pop")] + options,
                          cwd=os.path.dirname(proj), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)


def main():
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    proj = os.path.join(OUT, "proj")
    make_project(proj)
    for run, options in RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "proj")
            shutil.copytree(proj, p)
            r = run_reference(p, options)
            assert r.returncode == 0, r.stderr
            outdir = [d for d in os.listdir(p) if d.startswith("distances")]
            assert len(outdir) == 1, outdir
            shutil.copytree(os.path.join(p, outdir[0]), os.path.join(OUT, "expected", run))
    w(os.path.join(OUT, "runs.json"), json.dumps({run: {"options": o, "outdir": "distances-m5-d2" + (".matched_pos" if "--matched" in o else "")}
                                                  for run, o in RUNS.items()}, indent=1, sort_keys=True))
    # a species without S rows: the reference raises in computeDivNS
    nos = os.path.join(OUT, "noS", "proj")
    rnd = random.Random(7)
    text = "\t" + "\t".join(SAMPLES[:3]) + "\n"
    for k in range(40):
        text += "spN.c:-:%d:A>T:%s\t%s\n" % (k + 1, rnd.choice(["N[ATG-ACG]", "."]), "\t".join(value(rnd, .1) for _ in range(3)))
    w(os.path.join(nos, PARS, "pop", "spN.filtered.freq"), text)
    for name, head in (("proj.all_cov.tab", "Average_cov"), ("proj.all_perc.tab", "Percentage_1x")):
        w(os.path.join(nos, name), "\t" + "\t".join(SAMPLES[:3]) + "\nTaxId\t" + "\t".join([head] * 3) + "\nspN\t5.000000\t6.000000\t7.000000\n")
    w(os.path.join(nos, "bed_header"), "spN.c\t1\t1000\n")
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "proj")
        shutil.copytree(nos, p)
        r = run_reference(p, ["--divNS"])
    w(os.path.join(OUT, "noS", "result.json"), json.dumps({"options": ["--divNS"], "reference_fails": r.returncode != 0,
                                                          "message": "can't seem to find either type of SNV" if "find either type of SNV" in r.stderr else None},
                                                         indent=1, sort_keys=True))
    print("goldens written to", OUT)


if __name__ == "__main__":
    main()
