#!/usr/bin/env python
"""metaSNV_DistDiv.py --div on one synthetic species table through the entry point (msnv_div_file via
metasnv_amd.distdiv.compute_div): 160 samples x 100 000 positions, about 10 % of them multi-allelic (2 or 3 rows),
20 % of the values missing.  Prints and writes one JSON: the kernels' time (the entry's out-parameter), the wall time
of the call, and the driver's own share (coverage tables, bed_header, row order).
    timeout -k 10 300 python profiles/div_time.py [--samples 160] [--positions 100000] [--out profiles/div_time_160x100k.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(proj, S, P, seed=1):
    rng = np.random.default_rng(seed)
    pop = os.path.join(proj, "filtered", "pop")
    os.makedirs(pop)
    names = ["s%03d.bam" % i for i in range(S)]
    m = np.where(rng.random(P) < 0.1, rng.choice([2, 3], P), 1)       # rows per position
    n_rows = int(m.sum())
    pool = [repr(k / c) for c in (2, 3, 7, 40, 97, 1000, 29989) for k in range(0, c + 1, max(1, c // 40))]
    pool = np.array(pool + ["-1"] * (len(pool) // 4))                   # 20 % missing
    cells = pool[rng.integers(0, len(pool), (n_rows, S))]
    syn = np.array(["N[ATG-ACG]", "S[GCT-GCC]", "."])
    with open(os.path.join(pop, "spX.filtered.freq"), "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        r = 0
        for p in rng.permutation(P):
            for k in range(m[p]):
                f.write("spX.c%d:-:%d:A>%s:%s\t" % (p % 7, p + 1, "CGT"[k], syn[(p + k) % 3]) + "\t".join(cells[r]) + "\n")
                r += 1
    for tab, head in (("proj.all_cov.tab", "Average_cov"), ("proj.all_perc.tab", "Percentage_1x")):
        with open(os.path.join(proj, tab), "w") as f:
            f.write("\t" + "\t".join(names) + "\nTaxId\t" + "\t".join([head] * S) + "\n")
            f.write("spX\t" + "\t".join("%f" % x for x in rng.uniform(2, 90, S)) + "\n")
    with open(os.path.join(proj, "bed_header"), "w") as f:
        f.write("".join("spX.c%d\t1\t%d\n" % (c, 300000) for c in range(7)))
    return os.path.join(pop, "spX.filtered.freq"), n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=160)
    ap.add_argument("--positions", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from metasnv_amd import core, distdiv
    from metasnv_amd._lib import DIV
    with tempfile.TemporaryDirectory() as tmp:
        proj = os.path.join(tmp, "proj")
        t0 = time.perf_counter()
        freq, n_rows = synth(proj, a.samples, a.positions)
        t_synth = time.perf_counter() - t0
        outdir = os.path.join(proj, "distances")
        os.makedirs(outdir)
        ctx = core.Context(0)
        runs = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            tabs = (distdiv.read_tab(os.path.join(proj, "proj.all_perc.tab")), distdiv.read_tab(os.path.join(proj, "proj.all_cov.tab")),
                    distdiv.genome_lengths(os.path.join(proj, "bed_header")))
            t1 = time.perf_counter()
            distdiv.row_order(freq, stable=False)              # what compute_div does first, timed on its own
            t2 = time.perf_counter()
            ns, nr, ms = distdiv.compute_div(ctx, freq, DIV, False, tabs, outdir)
            t3 = time.perf_counter()
            runs.append({"tables_ms": (t1 - t0) * 1e3, "row_order_ms": (t2 - t1) * 1e3, "compute_div_wall_ms": (t3 - t2) * 1e3, "kernel_ms": ms})
        ctx.close()
        res = {"what": "metaSNV_DistDiv.py --div, one species table, msnv_div_file", "samples": ns, "rows": nr, "positions": a.positions,
               "pairs": ns * (ns + 1) // 2, "freq_bytes": os.path.getsize(freq), "synth_s": round(t_synth, 2), "runs": runs,
               "kernel_ms_min": min(r["kernel_ms"] for r in runs), "compute_div_wall_ms_min": min(r["compute_div_wall_ms"] for r in runs)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
