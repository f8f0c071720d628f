#!/usr/bin/env python
"""The row order of the report heatmaps (msnv_heatmap_file, msnv_hclust_tasks via metasnv_amd.subpopr) at three sizes: the file stage at 200 and
at 1000 samples (every sample with average linkage and a discovery subset of nine tenths with complete linkage, one launch of two workgroups),
and one task of 4096 members, the cap.  Prints and writes one JSON: the kernel's time from hip events and the stage's wall time (warm-up, then
the median of --repeat runs) and, for orientation only, the time scipy's linkage takes for the same trees on this machine's CPU.
    timeout -k 10 600 python profiles/hclust_time.py [--out profiles/hclust_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def manhattan(n, seed, dims=16):
    """Sum of |x_i - x_j| over a few coordinates of points around three centres, one coordinate at a time (128 MB at n = 4096)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 100, size=(3, dims))
    p = centres[np.arange(n) % 3] + rng.normal(0, 30.0, size=(n, dims))
    d = np.zeros((n, n))
    for c in range(dims):
        d += np.abs(p[:, c, None] - p[None, :, c])
    return d


def scipy_ms(d, method):
    try:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
    except ImportError:
        return None
    v = squareform(d, checks=False)
    t0 = time.perf_counter()
    linkage(v, method=method)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pamcases as cases
    from metasnv_amd import core, subpopr
    from metasnv_amd._lib import HCLUST_AVERAGE
    ctx = core.Context(0)
    out = {"what": "msnv_heatmap_file (all samples / average + nine tenths / complete) and one msnv_hclust_tasks task of 4096 members"}
    for n in (200, 1000):
        names = cases.sample_names(n)
        d = manhattan(n, n)
        sub = sorted(np.random.default_rng(n).permutation(n)[:n * 9 // 10].tolist())
        with tempfile.TemporaryDirectory() as tmp:
            dist_path = os.path.join(tmp, "sp.filtered.mann.dist")
            cases.write_dist(dist_path, names, d)
            with open(os.path.join(tmp, "sp_mann_distMatrixUsedForClustMedoidDefns.txt"), "w") as f:      # the stage reads the header's names alone
                f.write("\t".join(names[i] for i in sub) + "\n")
            with open(os.path.join(tmp, "sp_mann_clustering.tab"), "w") as f:
                f.write("clust\n" + "".join("%s\t%d\n" % (names[i], 1 + i % 3) for i in sub))
            subpopr.heatmap_file(ctx, dist_path, tmp)
            wall, ms = [], []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                res = subpopr.heatmap_file(ctx, dist_path, tmp)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(res["ms_kernel"])
        cpu = [scipy_ms(d, "average"), scipy_ms(d[np.ix_(sub, sub)], "complete")]
        out["stage_%d" % n] = {"samples": n, "discovery": len(sub), "kernel_ms": ms, "kernel_ms_median": float(np.median(ms)), "wall_ms_median": float(np.median(wall)),
                               "scipy_linkage_ms": None if None in cpu else cpu[0] + cpu[1]}
    n = 4096
    d = manhattan(n, n)
    subpopr.hclust_tasks(ctx, d[:64, :64], [(np.arange(64), HCLUST_AVERAGE)])
    ms = [subpopr.hclust_tasks(ctx, d, [(np.arange(n), HCLUST_AVERAGE)])[1] for _ in range(3)]
    out["task_4096"] = {"members": n, "method": "average", "kernel_ms": ms, "kernel_ms_median": float(np.median(ms)), "scipy_linkage_ms": scipy_ms(d, "average")}
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
