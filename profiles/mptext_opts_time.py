"""measure_ms / write_ms (mpileup_stats, whole milliseconds) of the mpileup-text kernels on one synth cohort, for an A/B of two builds and
for the options of msnv_mpileup_text_opts (MEASURED.md, "`msnv_mpileup_text_opts`").

  MODE=old   calls msnv_mpileup_text_records: works with a library from before the options too (MSNV_LIBRARY=<that libmsnv.so>)
  MODE=new   calls msnv_mpileup_text_records_ex with OPTS=all_positions,output_mq,output_bp
  CONTIG, COV, REPS: contig length (600000), mean coverage (10) and timed calls (5, behind one warm-up) of the 16-sample, 2-contig cohort

For kernel times finer than a millisecond run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python ...`."""
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from metasnv_amd import core, _lib
from parity import synth_case

mode = os.environ.get("MODE", "old")
opts = tuple(int(x) for x in os.environ.get("OPTS", "0,0,0").split(","))
reps = int(os.environ.get("REPS", "5"))
syn, samples = synth_case(n_species=2, contig_len=int(os.environ.get("CONTIG", "600000")), n_samples=16, mean_cov=float(os.environ.get("COV", "10")), seed=5)
n = len(syn.names)
names = (C.c_char_p * n)(*[s.encode() for s in syn.names])
lengths = (C.c_int64 * n)(*syn.lengths)
seqs = (C.c_char_p * n)(*[s.encode() if isinstance(s, str) else s for s in syn.seqs])
seq_lens = (C.c_int64 * n)(*[len(s) for s in syn.seqs])
rd = _lib.RefDesc(n, names, lengths, seqs, seq_lens)
p = core.default_params()
bufs = [np.ascontiguousarray(s, dtype=np.uint8) for s in samples]
ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data if b.size else None for b in bufs])
sizes = (C.c_uint64 * len(bufs))(*[b.size for b in bufs])
ctx = core.Context(0)
digest = None


def run():
    global digest
    text, nb, st = C.POINTER(C.c_char)(), C.c_uint64(), (C.c_uint64 * 8)()
    t0 = time.time()
    if mode == "old":
        _lib.check(_lib.lib.msnv_mpileup_text_records(ctx._h, C.byref(rd), C.byref(p), 0, None, None, None, ptrs, sizes, len(bufs), C.byref(text), C.byref(nb), st))
    else:
        o = _lib.MpileupTextOpts(opts[0], opts[1], opts[2], 0)
        _lib.check(_lib.lib.msnv_mpileup_text_records_ex(ctx._h, C.byref(rd), C.byref(p), C.byref(o), 0, None, None, None, ptrs, sizes, len(bufs), C.byref(text),
                                                         C.byref(nb), st))
    wall = time.time() - t0
    if digest is None:
        digest = hashlib.md5(C.string_at(text, nb.value)).hexdigest()
    _lib.lib.msnv_free(text)
    return int(st[4]), int(st[5]), int(st[2]), int(st[0]), wall


run()
res = [run() for _ in range(reps)]
print("TIMING lib=%s mode=%s opts=%s measure_ms=%s write_ms=%s text_bytes=%d lines=%d md5=%s wall=%s" % (
    os.path.basename(os.path.dirname(_lib.LIB_PATH)), mode, opts, [r[0] for r in res], [r[1] for r in res], res[0][2], res[0][3], digest,
    ["%.2f" % r[4] for r in res]), flush=True)
ctx.close()
