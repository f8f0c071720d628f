"""profiles/mptext_time.py -- msnv_mpileup_text on BASELINE configs[1]'s shape reduced to NS samples (default 16): 3 x 300 kb, ~10x.
Median of 10 runs after 3 warm-ups of BAM files -> text on /dev/null: wall seconds, the measure / write kernel ms and text bytes of `stats`;
once, the oracle's formatter on one core on the same records (the only other producer of the text) with a byte comparison of the two
texts; and, in a child process of its own (nothing else running), the device-to-host copy of the same number of bytes.
Run from the repository root: python3 profiles/mptext_time.py [out.json]"""
import ctypes as C, hashlib, json, os, statistics, subprocess, sys, tempfile, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from metasnv_amd import core
import orc

D2H = """
import statistics, sys, time, torch
n = int(sys.argv[1]); d = torch.empty(n, dtype=torch.uint8, device="cuda"); h = torch.empty(n, dtype=torch.uint8).pin_memory(); t = []
for i in range(13):
    torch.cuda.synchronize(); t0 = time.perf_counter(); h.copy_(d, non_blocking=True); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
print(statistics.median(t[3:]))
"""

ns = int(os.environ.get("NS", "16"))
sp = core.synth_params(n_species=3, contig_len=300000, n_samples=ns, mean_cov=float(os.environ.get("COV", "10")), seed=1)
syn = core.Synth(sp)
samples = [syn.sample_records(i) for i in range(ns)]
res = {"samples": ns, "record_bytes": int(sum(s.size for s in samples))}
with tempfile.TemporaryDirectory() as td:
    fa = os.path.join(td, "ref.fa"); syn.write_fasta(fa)
    paths = []
    for i, s in enumerate(samples):
        paths.append(os.path.join(td, "s%d.bam" % i)); core.write_bam(paths[-1], syn.names, syn.lengths, s)
    ctx = core.Context(0)
    wall, st = [], []
    for i in range(13):
        t0 = time.perf_counter(); st.append(ctx.mpileup_files(paths, fa, "/dev/null")); wall.append(time.perf_counter() - t0)
    wall, st = wall[3:], st[3:]
    res.update(text_bytes=st[0]["text_bytes"], lines=st[0]["lines"], elements=st[0]["elements"], batches=st[0]["batches"],
               wall_s_median=statistics.median(wall), wall_s_min=min(wall), wall_s_max=max(wall),
               measure_ms_median=statistics.median(s["measure_ms"] for s in st), write_ms_median=statistics.median(s["write_ms"] for s in st))
    res["end_to_end_bytes_per_s"] = res["text_bytes"] / res["wall_s_median"]
    res["kernel_bytes_per_s"] = res["text_bytes"] / ((res["measure_ms_median"] + res["write_ms_median"]) / 1e3)
    # records already in memory (no file read, no inflate): what is left is the pre-pass, the uploads and the device
    t0 = time.perf_counter(); text = ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples); res["from_records_wall_s"] = time.perf_counter() - t0
    ctx.close()
    # the oracle on one core, same records
    ref = orc.make_ref(syn.names, syn.lengths, syn.seqs); smp = orc.make_samples(samples); mo, _ = orc.mp_opts(None)
    op = os.path.join(td, "oracle.mp")
    t0 = time.perf_counter(); rc = orc.lib().orc_mpileup_to_file(C.byref(ref.ref), smp.arr, len(smp.bufs), C.byref(mo), op.encode()); res["oracle_one_core_s"] = time.perf_counter() - t0
    assert rc == 0
    h = hashlib.sha256()
    with open(op, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    res["text_equals_oracle"] = h.digest() == hashlib.sha256(text).digest()
    res["oracle_bytes_per_s"] = res["text_bytes"] / res["oracle_one_core_s"]
r = subprocess.run([sys.executable, "-c", D2H, str(res["text_bytes"])], capture_output=True, text=True, timeout=600)
res["d2h_s_median"] = float(r.stdout.strip()) if r.returncode == 0 else None
res["d2h_bytes_per_s"] = res["text_bytes"] / res["d2h_s_median"] if res["d2h_s_median"] else None
print(json.dumps(res))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(json.dumps(res, indent=1) + "\n")
