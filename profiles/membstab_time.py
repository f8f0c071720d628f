#!/usr/bin/env python
"""subpopr's membership-stability stage (msnv_membership_stability_file via metasnv_amd.subpopr.membership_stability_file) at 200 samples in 3
planted groups with the default 100 subsets at each of 8 proportions: 801 PAM runs and 800 matchings in two launches.  Prints and writes one
JSON: the stage's wall time and its kernels' time from hip events (warm-up, then the median of --repeat runs), with the cluster stage on the
same matrix beside it.
    timeout -k 10 300 python profiles/membstab_time.py [--samples 200] [--out profiles/membstab_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pamcases as cases
    from metasnv_amd import core, subpopr
    n = a.samples
    ctx = core.Context(0)
    out = {"what": "msnv_membership_stability_file: 100 subsets per proportion, PAM and matching", "samples": n}
    with tempfile.TemporaryDirectory() as tmp:
        dist_path = os.path.join(tmp, "sp.filtered.mann.dist")
        cases.write_dist(dist_path, cases.sample_names(n), cases.planted_dist(n, 3, 1))
        stage = os.path.join(tmp, "stage")
        subpopr.cluster_file(ctx, dist_path, os.path.join(tmp, "warm"), stability_iters=1)
        t0 = time.perf_counter()
        res = subpopr.cluster_file(ctx, dist_path, stage)
        out.update(cluster_stage_wall_ms=(time.perf_counter() - t0) * 1e3, cluster_stage_kernel_ms=res["ms_kernel"])
        k = subpopr.clusters_from_ps_values(stage, "sp")
        prefix = os.path.join(stage, "sp_mann")
        args = (ctx, prefix + "_distMatrixUsedForClustMedoidDefns.txt", "sp", k)
        subpopr.membership_stability_file(*args, os.path.join(tmp, "warm"), boot_iters=1)
        wall, ms = [], []
        for r in range(a.repeat):
            t0 = time.perf_counter()
            res = subpopr.membership_stability_file(*args, os.path.join(tmp, "out%d" % r), clus_num_stability_path=prefix + "_clusNumStability.tab")
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(res["ms_kernel"])
        out["assessment"] = open(os.path.join(tmp, "out0", "sp_mann_stabilityAssessment.tab")).read()
    out.update(stage_wall_ms=wall, stage_wall_ms_median=float(np.median(wall)), stage_kernel_ms=ms, stage_kernel_ms_median=float(np.median(ms)), k=k,
               n_sets=res["n_sets"], n_proportions=res["n_proportions"])
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
