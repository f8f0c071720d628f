#!/usr/bin/env python
"""subpopr's gene-profile correlations through the array entry (msnv_gene_corr via metasnv_amd.subpopr.gene_correlations) at the shape the
reference's manual quotes: 7 524 samples x 136 000 gene families x (4 clusters + the species row), seeded numpy data, 70 % zeros.
Prints and writes one JSON: the kernels' time from hip events (the entry's out-parameter; warm-up, then the median of --repeat calls),
the wall time of a call (which uploads the matrix each time), the gene matrix's bytes over the kernel time against 8 TB/s, and the
numpy model's time (tests/genecorrmodel.py) on every --model-stride'th row, scaled.
    timeout -k 10 900 python profiles/genecorr_time.py [--samples 7524] [--genes 136000] [--clusters 4] [--out profiles/genecorr_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7524)
    ap.add_argument("--genes", type=int, default=136000)
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--model-stride", type=int, default=100, help="0: skip the numpy model")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from metasnv_amd import core, subpopr
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    genes = np.empty((a.genes, a.samples))
    for lo in range(0, a.genes, 8192):                            # block by block: no second copy of 8 GB
        blk = genes[lo:lo + 8192]
        blk[:] = np.exp(rng.normal(0.0, 2.0, blk.shape))
        blk[rng.random(blk.shape) < 0.7] = 0.0
    clust = np.exp(rng.normal(-2.0, 1.0, (a.clusters + 1, a.samples)))
    clust[:-1][rng.random((a.clusters, a.samples)) < 0.5] = 0.0
    clust[-1] = clust[:-1].sum(axis=0)
    t_synth = time.perf_counter() - t0
    ctx = core.Context(0)
    subpopr.gene_correlations(ctx, clust, genes)                  # warm-up
    ms, wall = [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        res = subpopr.gene_correlations(ctx, clust, genes)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(res["ms_kernel"])
    ctx.close()
    out = {"what": "msnv_gene_corr: ranks + Spearman + Pearson of every (cluster, gene) pair", "samples": a.samples, "genes": a.genes,
           "cluster_rows": a.clusters + 1, "zero_share": 0.7, "synth_s": round(t_synth, 1), "kernel_ms": ms, "kernel_ms_median": float(np.median(ms)),
           "call_wall_ms_median": float(np.median(wall)), "gene_matrix_bytes": int(genes.nbytes), "valid_pairs": int(res["valid"].sum())}
    # the matrix is read twice (the pseudocount pass, then the rows): bytes / time of ONE reading against the 8 TB/s the project quotes for HBM
    out["matrix_bytes_per_s"] = genes.nbytes / (out["kernel_ms_median"] * 1e-3)
    out["share_of_8TBps"] = out["matrix_bytes_per_s"] / 8e12
    if a.model_stride > 0:
        import genecorrmodel as model
        sub = genes[::a.model_stride]
        t0 = time.perf_counter()
        want = model.gene_correlations(clust, sub)
        t_model = time.perf_counter() - t0
        ok = want["valid"]
        out["model_rows"] = int(sub.shape[0])
        out["model_s"] = round(t_model, 2)
        out["model_s_scaled_to_all_rows"] = round(t_model * a.genes / sub.shape[0], 1)
        # the sample's pseudocount is its own smallest cell: compare rho (which does not depend on it) and r only where the pseudocounts agree
        out["worst_abs_rho_vs_model"] = float(np.abs(res["rho"][:, ::a.model_stride][ok] - want["rho"][ok]).max())
        if want["pseudocount"] == res["pseudocount"]:
            out["worst_abs_r_vs_model"] = float(np.abs(res["r"][:, ::a.model_stride][ok] - want["r"][ok]).max())
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
