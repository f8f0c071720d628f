#!/usr/bin/env python
"""subpopr's clustering stage (msnv_cluster_file via metasnv_amd.subpopr.cluster_file) at the size the issue names: 200 samples in 3 planted
groups, the default M = 50 and 10 stability subsamples per proportion -- 1 400 + 72 000 PAM runs and their classification.  Prints and writes
one JSON: the stage's wall time and its kernels' time from hip events (warm-up, then the median of --repeat runs), and what bounds the PAM
kernel: the same --tasks tasks (half-size subsets, k = 2..10) timed on the 200 x 200 matrix (320 KB, resident in L2) and on the same distances
spread over a 4096 x 4096 matrix (every cell on a cache line of its own, 128 MB behind them).
    timeout -k 10 600 python profiles/cluster_time.py [--samples 200] [--out profiles/cluster_time.json]
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
    ap.add_argument("--tasks", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pamcases as cases
    from metasnv_amd import core, subpopr
    n = a.samples
    names = cases.sample_names(n)
    d = cases.planted_dist(n, 3, 1)
    ctx = core.Context(0)
    out = {"what": "msnv_cluster_file: prediction strength (M = 50), PAM, cluster-number stability (10 subsamples per proportion)", "samples": n}
    with tempfile.TemporaryDirectory() as tmp:
        dist_path = os.path.join(tmp, "sp.filtered.mann.dist")
        cases.write_dist(dist_path, names, d)
        subpopr.cluster_file(ctx, dist_path, os.path.join(tmp, "warm"), stability_iters=1)
        wall, ms = [], []
        for r in range(a.repeat):
            t0 = time.perf_counter()
            res = subpopr.cluster_file(ctx, dist_path, os.path.join(tmp, "out%d" % r))
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(res["ms_kernel"])
    out.update(stage_wall_ms=wall, stage_wall_ms_median=float(np.median(wall)), stage_kernel_ms=ms, stage_kernel_ms_median=float(np.median(ms)),
               pam_tasks=res["n_pam_tasks"], n_clusters=res["n_clusters"], stability_score=res["stability_score"])
    # what bounds the PAM kernel: the same tasks, the matrix in L2 or spread over 128 MB
    rng = np.random.default_rng(3)
    m = n // 2
    tasks = [(rng.choice(n, size=m, replace=False).astype(np.int32), 2 + t % 9) for t in range(a.tasks)]
    stride = 4096 // n
    big = np.zeros((4096, 4096))
    spread = np.arange(n) * stride
    big[np.ix_(spread, spread)] = d
    far = [((ix * stride).astype(np.int32), k) for ix, k in tasks]
    for label, mat, tk in (("resident", d, tasks), ("spread", big, far)):
        subpopr.pam_tasks(ctx, mat, tk[:64])
        t = [subpopr.pam_tasks(ctx, mat, tk)[1] for _ in range(3)]
        out["pam_%s_kernel_ms" % label] = t
        out["pam_%s_tasks_per_s" % label] = a.tasks / (float(np.median(t)) * 1e-3)
    out["pam_task_members"], out["pam_task_count"] = m, a.tasks
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
