#!/usr/bin/env python
"""The read subsampler (msnv_records_subsample_device, csrc/devsub.hip) next to its yardstick, the device dealer with ONE part
(msnv_records_deal_device, csrc/devdeal.hip), on the same device-resident record streams on the same box: both stage the streams, run the
record scan, decide per record and copy the survivors; the dealer sorts the records by owner in between, the subsampler hashes their names.
Streams: --samples synthetic samples of core.Synth (a few million records in all).  Per call the wall time (median of --repeat, after a
warm-up) and, for the subsampler, the kernel milliseconds the library reports (record scan + measure + size scan + copy, HIP events).  The
dealer reports no kernel time: what is printed for it is its wall time less the subsampler's non-kernel share (staging copies, allocations,
the small downloads -- the same work in both calls), an ESTIMATE; `rocprofv3 --kernel-trace --stats -- python profiles/subsample_time.py`
gives the per-kernel sums of both.  Bytes moved: the record bytes read (every stream once by the staging copy, once by the scan and the
decision's header loads in part, once by the copy for what survives) and the bytes the copy writes.  Prints and writes one JSON.
    timeout -k 10 900 python profiles/subsample_time.py [--out profiles/subsample_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--species", type=int, default=100)
    ap.add_argument("--contig-len", type=int, default=20000)
    ap.add_argument("--mean-cov", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from metasnv_amd import _lib, core
    ctx = core.Context(0)
    hip = C.CDLL("libamdhip64.so")
    sp = core.synth_params(n_species=a.species, contig_len=a.contig_len, n_samples=a.samples, mean_cov=a.mean_cov, snv_density=0.01, frac_paired=0.5, seed=11)
    syn = core.Synth(sp)
    t0 = time.perf_counter()
    streams = [np.ascontiguousarray(syn.sample_records(i), dtype=np.uint8) for i in range(a.samples)]
    synth_s = time.perf_counter() - t0
    sizes = [int(s.size) for s in streams]
    total = sum(sizes)
    ptrs = []
    for s in streams:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(16, s.size))) == 0
        assert hip.hipMemcpy(p, C.c_void_p(s.ctypes.data), C.c_size_t(s.size), 1) == 0
        ptrs.append(p.value)
    n = len(ptrs)
    cap = sum((x + 31) & ~15 for x in sizes) + 256
    out_buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(out_buf), C.c_size_t(cap)) == 0
    pa = (C.c_void_p * n)(*ptrs); sa = (C.c_uint64 * n)(*sizes)
    oo = (C.c_uint64 * n)(); ob = (C.c_uint64 * n)(); cn = (C.c_uint64 * (2 * n))(); ms = C.c_double()
    word = core.subsample_seed_word(42)

    def sub(frac):
        t0 = time.perf_counter()
        _lib.check(_lib.lib.msnv_records_subsample_device(ctx._h, pa, sa, n, 1, word, frac, out_buf, cap, oo, ob, cn, C.byref(ms)))
        return (time.perf_counter() - t0) * 1e3, ms.value, sum(ob[i] for i in range(n)), sum(cn[2 * i] for i in range(n)), sum(cn[2 * i + 1] for i in range(n))

    owner = np.zeros(len(syn.names), dtype=np.int32)

    def deal():
        t0 = time.perf_counter()
        pb, st = core.deal_records_device(ctx, ptrs, owner, 1, out_buf.value, cap, on_device=True, sizes=sizes)
        return (time.perf_counter() - t0) * 1e3, int(pb.sum())

    sub(.5); deal()                                               # warm-up: code objects, the allocator's cache
    res = {"what": "msnv_records_subsample_device against msnv_records_deal_device with one part, same device-resident streams", "streams": n, "record_bytes": total,
           "synth_wall_s": synth_s, "repeat": a.repeat}
    overhead = []
    for frac in (.5, 1.0):
        runs = [sub(frac) for _ in range(a.repeat)]
        wall, kern = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
        overhead.append(wall - kern)
        res["subsample_frac_%g" % frac] = {"wall_ms": [r[0] for r in runs], "wall_ms_median": wall, "kernel_ms": [r[1] for r in runs], "kernel_ms_median": kern,
                                           "records_kept": int(runs[0][3]), "records_dropped": int(runs[0][4]), "bytes_written": int(runs[0][2]),
                                           "bytes_read_staging": total, "bytes_read_copy": int(runs[0][2])}
    runs = [deal() for _ in range(a.repeat)]
    wall = float(np.median([r[0] for r in runs]))
    res["deal_one_part"] = {"wall_ms": [r[0] for r in runs], "wall_ms_median": wall, "kernel_ms_estimate": wall - float(np.mean(overhead)), "bytes_written": runs[0][1],
                            "bytes_read_staging": total, "bytes_read_copy": runs[0][1]}
    res["records"] = res["subsample_frac_1"]["records_kept"]
    for p in ptrs:
        hip.hipFree(C.c_void_p(p))
    hip.hipFree(out_buf)
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
