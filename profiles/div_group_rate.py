#!/usr/bin/env python
"""How fast ONE lane of msnv_div_pairs sums the k x k outer product of one multi-allelic group (k = m(m-1)+1): a table that
is one group of m rows and one sample (one pair, one working lane), through msnv_div_file, the entry's ms_kernel, three runs
each for m = 13 and m = 24.  The rate per product, and the largest m whose k^2 products stay under one second per pair at that
rate -- the device side of DIV_MAX_ALLELES (csrc/device.h).  Prints and writes one JSON.
    timeout -k 10 120 python profiles/div_group_rate.py [--out profiles/div_group_rate.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import divcases
    from metasnv_amd import core
    ctx = core.Context(0)
    res = {"what": "msnv_div_pairs, one group of m rows, one sample: ms_kernel of msnv_div_file", "runs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        empty = divcases.one_group(2, 1)
        res["runs"]["m=2"] = [divcases.device_outputs(ctx, empty, tmp)[1] for _ in range(4)][1:]      # the launch itself (first call: code load)
        for m in (13, 24):
            case = divcases.one_group(m, 7)
            res["runs"]["m=%d" % m] = [divcases.device_outputs(ctx, case, tmp)[1] for _ in range(3)]
    ctx.close()
    k2 = lambda m: (m * (m - 1) + 1) ** 2
    t13, t24 = min(res["runs"]["m=13"]), min(res["runs"]["m=24"])
    res["products"] = {"m=13": k2(13), "m=24": k2(24)}
    res["ns_per_product"] = {"m=13": t13 * 1e6 / k2(13), "m=24": t24 * 1e6 / k2(24), "slope": (t24 - t13) * 1e6 / (k2(24) - k2(13))}
    rate = max(res["ns_per_product"].values())                  # the slower figure bounds the time from above
    res["largest_m_under_one_second"] = max(m for m in range(2, 2000) if k2(m) * rate < 1e9)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
