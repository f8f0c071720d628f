#!/usr/bin/env python
"""Generates tests/golden/python_callers/dist_long/* by RUNNING the reference's metaSNV_DistDiv.py --dist from
/root/reference on tables far longer than a committed file may be.  Only what the reference wrote is kept:

  <case>/<case>.filtered.mann.dist, .allele.dist    a few hundred bytes to a few hundred kilobytes
  cases.json                                       per case: the arguments of tests/distmodel.py make_table (seed, shape,
                                                   NaN rates ...), the options, the output directory and the sha256 of the table

The tests regenerate every table with the same make_table, check the sha256 and compare bytes; no input table is stored.
Re-run in the build container:  python tests/golden/make_dist_long_goldens.py

  n8193x4          one row past numpy's 8192-element summation block
  n20000x7         three blocks, run through the driver
  n20000x7_matched --dist --matched (the reference's --dist does not filter the rows: only the directory changes); NaN
                   rates that leave > 8192 rows even under filt_proportion
  n300000x3        past the kernel's LDS / scratch crossover
  n3000x70         2 485 pairs; smp5 all NaN (an empty row and column of .mann.dist, 0.0 in .allele.dist), smp9 = smp3
                   (a distance of exactly 0.0)
Every table has a NaN-heavy sample (smp1).
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "python_callers", "dist_long")
sys.path.insert(0, os.path.dirname(HERE))
import distmodel  # noqa: E402

CASES = {
    "n8193x4": {"table": {"seed": 101, "n_pos": 8193, "S": 4}, "options": ["--dist"]},
    "n20000x7": {"table": {"seed": 102, "n_pos": 20000, "S": 7}, "options": ["--dist"]},
    "n20000x7_matched": {"table": {"seed": 103, "n_pos": 20000, "S": 7, "nan_rates": [.02, .3, .02, .02, .02, .02, .02]}, "options": ["--dist", "--matched"]},
    "n300000x3": {"table": {"seed": 107, "n_pos": 300000, "S": 3}, "options": ["--dist"]},
    "n3000x70": {"table": {"seed": 105, "n_pos": 3000, "S": 70, "all_nan": 5, "same_as": [3, 9]}, "options": ["--dist"]},
}


def main():
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    meta = {}
    for case, spec in CASES.items():
        names, text = distmodel.make_table(**spec["table"])
        with tempfile.TemporaryDirectory() as tmp:
            proj = os.path.join(tmp, "proj")
            pop = distmodel.write_project(proj, case, text)
            r = subprocess.run([sys.executable, os.path.join(REF, "metaSNV_DistDiv.py"), "--filt", pop] + spec["options"], cwd=tmp,
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stderr
            outdir = [d for d in os.listdir(proj) if d.startswith("distances")]
            assert len(outdir) == 1, outdir
            shutil.copytree(os.path.join(proj, outdir[0]), os.path.join(OUT, case))
        assert sorted(os.listdir(os.path.join(OUT, case))) == [case + ".filtered.allele.dist", case + ".filtered.mann.dist"]
        meta[case] = {"table": spec["table"], "options": spec["options"], "outdir": outdir[0], "sha256": hashlib.sha256(text.encode()).hexdigest()}
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write(json.dumps(meta, indent=1, sort_keys=True) + "\n")
    print("goldens written to", OUT)


if __name__ == "__main__":
    main()
