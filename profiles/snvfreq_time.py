#!/usr/bin/env python
"""The SNV-frequency curves (msnv_freq_curves via metasnv_amd.subpopr) next to their yardstick, the three fixed bands of msnv_freq_bands_k
(msnv_freq_bands), on the same tables: 200 000 x 500 and 2 000 000 x 100 cells of fp64.  Both kernels read every byte of the table once; the bands
kernel keeps four counters a thread, the curves kernel a hundred in LDS.  Kernel times are hip events around the launches alone (warm-up, then the
median of --repeat runs); GB/s is table bytes / kernel time.  Then the file stage (msnv_snvfreq_file) on a table of --stage-rows x 100 written as
text: its wall time, split into the kernel (events), the array call's remainder (allocation, upload, download: the wall time of msnv_freq_curves on
the same cells minus its kernel) and everything else (reading and parsing the text, the scaling, the two files).  Prints and writes one JSON.
    timeout -k 10 900 python profiles/snvfreq_time.py [--out profiles/snvfreq_time.json]
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


def table(n, S, seed):
    """Percent scale; three cells in four near an end, as filtered SNV tables are, one in seven without coverage."""
    rng = np.random.default_rng(seed)
    t = rng.random((n, S)) * 100.0
    end = rng.random((n, S))
    t = np.where(end < 0.375, t * 0.05, np.where(end < 0.75, 100.0 - t * 0.05, t))
    t[rng.random((n, S)) < 0.14] = np.nan
    return np.ascontiguousarray(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--stage-rows", type=int, default=50000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from metasnv_amd import core, subpopr
    ctx = core.Context(0)
    rows_per_block, lanes = subpopr.freq_curves_geometry()
    out = {"what": "msnv_freq_curves_k against msnv_freq_bands_k on the same table; then msnv_snvfreq_file", "rows_per_block": rows_per_block, "columns_per_block": lanes}
    subpopr.freq_curves(ctx, table(2048, 100, 1))
    subpopr.freq_bands(ctx, table(2048, 100, 1))
    for n, S in ((200000, 500), (2000000, 100)):
        t = table(n, S, n)
        curves, bands, wall = [], [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            curves.append(subpopr.freq_curves(ctx, t)["ms_kernel"])
            wall.append((time.perf_counter() - t0) * 1e3)
            bands.append(subpopr.freq_bands(ctx, t)[1])
        gb = t.nbytes / 1e9
        mc, mb = float(np.median(curves)), float(np.median(bands))
        out["%dx%d" % (n, S)] = {"rows": n, "samples": S, "table_gb": gb, "curves_kernel_ms": curves, "curves_kernel_ms_median": mc, "curves_gb_per_s": gb / (mc * 1e-3),
                                 "bands_kernel_ms": bands, "bands_kernel_ms_median": mb, "bands_gb_per_s": gb / (mb * 1e-3), "curves_over_bands": mc / mb,
                                 "curves_call_wall_ms_median": float(np.median(wall))}
        del t
    n, S = a.stage_rows, 100
    t = np.round(table(n, S, 7) / 100.0, 4)
    names = ["s%04d.bam" % (i + 1) for i in range(S)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sp.filtered.freq")
        with open(path, "w") as f:
            f.write("\t" + "\t".join(names) + "\n")
            for p in range(n):
                f.write("c1:-:%d:A:.\t" % (p + 1) + "\t".join("-1" if v != v else repr(v) for v in t[p].tolist()) + "\n")
        text_bytes = os.path.getsize(path)
        subpopr.snv_freq_file(ctx, path, tmp)
        stage, kernel, array = [], [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            res = subpopr.snv_freq_file(ctx, path, tmp)
            stage.append((time.perf_counter() - t0) * 1e3)
            kernel.append(res["ms_kernel"])
            t0 = time.perf_counter()
            ms = subpopr.freq_curves(ctx, t * 100.0)["ms_kernel"]
            array.append((time.perf_counter() - t0) * 1e3 - ms)
    w, k, u = float(np.median(stage)), float(np.median(kernel)), float(np.median(array))
    out["stage_%dx%d" % (n, S)] = {"rows": n, "samples": S, "text_mb": text_bytes / 1e6, "wall_ms_median": w, "kernel_ms_median": k, "alloc_upload_download_ms_median": u,
                                   "parse_scale_write_ms": w - k - u}
    ctx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
