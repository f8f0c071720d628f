"""The read subsampler on the device (`qaCompute -a`, `metaSNV.py --subsample`; csrc/devsub.hip): msnv_records_subsample_device against the
plain-Python model (tests/subsamplemodel.py) byte for byte, mates, a dataset that subsamples against a dataset built from the model's kept
records on both pack routes, the refusals, the msnv_qacompute drop-in and the launcher."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bamtools as bt
import subsamplemodel as sm
from metasnv_amd import _lib, core
from packsame import _env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools")
SIZES = (0, 1, 63, 64, 65, 257, 4096)
KEPT = {(0, .5): {64: 34, 257: 125, 4096: 2053}, (42, .25): {64: 17, 257: 64, 4096: 1041}, (7, .9): {64: 55, 257: 235, 4096: 3685},
        (42, 1e-7): {64: 0, 257: 0, 4096: 0}}
CIGAR40 = "".join("%d%s" % (1 + k % 3, "MIMD"[k % 4]) for k in range(39)) + "2M"      # 40 operations
CIGAR40_QUERY = sum(n for n, op in bt.parse_cigar(CIGAR40) if op in (0, 1, 4, 7, 8))      # bases of a read with that CIGAR


def _shaped(i, name, tid=0, pos=None, **kw):
    """Record i of a stream in one of four shapes: no SEQ, one CIGAR operation, 40 of them, aux data; lengths that walk through every
    residue of the record size modulo 16."""
    pos = 10 + i if pos is None else pos
    shape, n = i % 4, 1 + i % 17
    if shape == 0:
        return bt.make_record(tid, pos, "*", "*", name=name, flag=4 if i % 8 == 0 else 0, **kw)
    if shape == 1:
        return bt.make_record(tid, pos, "%dM" % n, ("ACGTTGCA" * 3)[:n], name=name, **kw)
    if shape == 2:
        return bt.make_record(tid, pos, CIGAR40, ("ACGT" * 40)[:CIGAR40_QUERY], name=name, **kw)
    return bt.make_record(tid, pos, "%dM" % n, ("GATTACA" * 3)[:n], name=name, aux=bt.aux_fields(nm=i % 5, md="%d" % n, score=-i) + b"XZZ" + b"y" * (i % 16) + b"\0", **kw)


@pytest.fixture(scope="module")
def named_streams():
    """Streams of SIZES records named r0 .. r{n-1} (the issue's count table), every shape among them."""
    out = {}
    for n in SIZES:
        out[n] = b"".join(_shaped(i, "r%d" % i) for i in range(n))
    assert len(out[4096]) > 256 * 1024                           # past a scan segment, and many sub-segments
    assert {sz % 16 for _, sz in sm.split_records(out[4096])} == set(range(16))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def _on_device(hip, streams):
    ptrs = []
    for s in streams:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(16, len(s)))) == 0
        if len(s):
            a = np.frombuffer(s, np.uint8)
            assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.size), 1) == 0
        ptrs.append(p.value)
    return ptrs


def _run(ctx, streams, seed, frac, where):
    arrs = [np.frombuffer(s, np.uint8) for s in streams]
    if where == "host":
        return core.subsample_records(ctx, arrs, seed, frac)
    hip = C.CDLL("libamdhip64.so")
    ptrs = _on_device(hip, streams)
    try:
        return core.subsample_records(ctx, ptrs, seed, frac, on_device=True, sizes=[len(s) for s in streams])
    finally:
        for p in ptrs:
            hip.hipFree(C.c_void_p(p))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("seed,frac", [(0, .5), (42, .25), (7, .9), (42, 1e-7), (42, 1.0)])
def test_array_form_equals_the_model_byte_for_byte(ctx, named_streams, seed, frac, where):
    """Several streams in one call, an empty one first, in the middle and last; the kept counts are the issue's table."""
    order = [0, 1, 63, 64, 0, 65, 257, 4096, 0]
    streams = [named_streams[n] for n in order]
    got, counts, ms = _run(ctx, streams, seed, frac, where)
    word = sm.seed_word(seed)
    for i, n in enumerate(order):
        want, kept, dropped = sm.filter_stream(streams[i], word, frac)
        print("n=%d seed=%d frac=%g kept=%d dropped=%d" % (n, seed, frac, kept, dropped))
        assert got[i] == want, (n, seed, frac)
        assert tuple(counts[i]) == (kept, dropped) and kept + dropped == n
        if frac == 1.0:
            assert got[i] == streams[i] and kept == n
        elif n in (64, 257, 4096):
            assert kept == KEPT[(seed, frac)][n]
    assert ms > 0


def test_no_fraction_means_no_launch(ctx, named_streams):
    streams = [named_streams[64], named_streams[257]]
    for frac in (0.0, -1.0):
        got, counts, ms = _run(ctx, streams, 42, frac, "host")
        assert got == streams and ms == 0 and not counts.any()
    # ... not even a look at the bytes: a stream that is no chain of records goes through
    got, counts, ms = _run(ctx, [b"\x01\x02\x03"], 42, 0.0, "host")
    assert got == [b"\x01\x02\x03"] and ms == 0


@pytest.mark.parametrize("where", ["host", "device"])
def test_names_of_every_length_and_bytes_above_0x7f(ctx, where):
    rnd = random.Random(77)
    lengths = [0, 1, 2, 31, 32, 33, 254]
    streams = []
    for n in (0, 1, 63, 64, 65, 257):
        recs = []
        for i in range(n):
            ln = lengths[i % len(lengths)]
            if i % 3 == 0:                                      # printable, as aligners write them
                nm = bytes(rnd.randrange(33, 127) for _ in range(ln))
            else:                                               # any byte but NUL, those of 0x80 and more (signed chars) among them
                nm = bytes(rnd.choice([rnd.randrange(1, 128), rnd.randrange(128, 256)]) for _ in range(ln))
            recs.append(sm.with_name(_shaped(i, "x" * ln), nm))
        streams.append(b"".join(recs))
    for seed, frac in ((0, .5), (42, .25), (7, .9)):
        got, counts, _ = _run(ctx, streams, seed, frac, where)
        total = 0
        for i, s in enumerate(streams):
            want, kept, dropped = sm.filter_stream(s, sm.seed_word(seed), frac)
            assert got[i] == want and tuple(counts[i]) == (kept, dropped), (i, seed, frac)
            total += kept
        assert 0 < total < sum(len(sm.split_records(s)) for s in streams)


def test_mates_share_a_fate(ctx):
    """Two records of one name at different positions of different contigs: both kept or both dropped, in streams of every size."""
    streams = []
    for n in SIZES:
        recs = []
        for i in range(n):
            j = i // 2
            recs.append(_shaped(i, "m%d" % j, tid=i % 2, pos=100 + 7 * i, mtid=1 - i % 2, mpos=100 + 7 * (i ^ 1), tlen=40, ))
        streams.append(b"".join(recs))
    for seed, frac in ((0, .5), (42, .25), (7, .9)):
        got, counts, _ = _run(ctx, streams, seed, frac, "host")
        for i, n in enumerate(SIZES):
            want, kept, _ = sm.filter_stream(streams[i], sm.seed_word(seed), frac)
            assert got[i] == want
            names = [sm.record_name(got[i], off) for off, _ in sm.split_records(got[i])]
            whole = n // 2                                       # (an odd stream's last record has no mate in it)
            paired = [nm for nm in names if int(nm[1:]) < whole]
            assert all(paired.count(nm) == 2 for nm in set(paired)), (n, seed, frac)
            if n >= 64:
                assert 0 < kept < n


def test_capacity_and_malformed_streams(ctx, named_streams):
    hip = C.CDLL("libamdhip64.so")
    s = np.frombuffer(named_streams[64], np.uint8)
    p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(1 << 16)) == 0
    pa = (C.c_void_p * 1)(s.ctypes.data); sa = (C.c_uint64 * 1)(s.size)
    oo = (C.c_uint64 * 1)(); ob = (C.c_uint64 * 1)(); cn = (C.c_uint64 * 2)(); ms = C.c_double()
    need = (s.size + 31) & ~15
    rc = _lib.lib.msnv_records_subsample_device(ctx._h, pa, sa, 1, 0, 5, .5, p, need - 1, oo, ob, cn, C.byref(ms))
    assert rc == _lib.EINVAL and ms.value == 0
    rc = _lib.lib.msnv_records_subsample_device(ctx._h, pa, sa, 1, 0, 5, .5, p, need, oo, ob, cn, C.byref(ms))
    assert rc == 0 and oo[0] == 0 and cn[0] + cn[1] == 64
    hip.hipFree(p)
    # a chain that breaks (the last record cut short) and a record whose CIGAR cannot fit its block_size: MSNV_EFORMAT, as in the dealer
    with pytest.raises(_lib.MsnvError) as e:
        core.subsample_records(ctx, [np.frombuffer(named_streams[64][:-3], np.uint8)], 42, .25)
    assert e.value.code == _lib.EFORMAT
    broken = bytearray(b"".join(bt.make_record(0, 5 + k, "10M", "ACGTACGTAC", name="b%d" % k) for k in range(3)))
    broken[16:18] = b"\xff\xff"
    with pytest.raises(_lib.MsnvError) as e:
        core.subsample_records(ctx, [np.frombuffer(bytes(broken), np.uint8)], 42, .25)
    assert e.value.code == _lib.EFORMAT


# ------------------------------------------------------------------------------------ through the dataset, the tool, the launcher
NAMES, LENGTHS = ["ctgA", "ctgB"], [1500, 1200]


def _reference():
    rnd = random.Random(3)
    return ["".join(rnd.choice("ACGT") for _ in range(n)) for n in LENGTHS]


def _cohort():
    """Three samples of 257 reads named r0 .. r256 (64 of them are kept at 42.25), 60 bases each, coordinate-sorted over two contigs, with
    a substituted base wherever the reference position is a multiple of 9 -- sites that the kept reads alone still call."""
    seqs = _reference()
    alt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    samples = []
    for s in range(3):
        recs = []
        for i in range(257):
            tid = 0 if i < 150 else 1
            pos = (i if tid == 0 else i - 150) * 5 + s
            ref = seqs[tid][pos:pos + 60]
            read = "".join(alt[c] if (pos + k) % 9 == 0 and (i + s) % 2 == 0 else c for k, c in enumerate(ref))
            recs.append(bt.make_record(tid, pos, "60M", read, name="r%d" % i, flag=1024 if i % 50 == 7 else 0, mapq=0 if i % 41 == 3 else 60))
        samples.append(b"".join(recs))
    return seqs, samples


def _write_cohort(d, samples):
    os.makedirs(d, exist_ok=True)
    paths = []
    for i, s in enumerate(samples):
        p = os.path.join(d, "s%d.bam" % i)
        core.write_bam(p, NAMES, LENGTHS, np.frombuffer(s, np.uint8))
        paths.append(p)
    return paths


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """X (all reads) and X' (the model's kept reads at seed 42, frac .25) as BAM files of the same names in two directories."""
    seqs, samples = _cohort()
    word = sm.seed_word(42)
    kept = []
    for s in samples:
        k, n_kept, _ = sm.filter_stream(s, word, .25)
        assert n_kept == 64
        kept.append(k)
    root = tmp_path_factory.mktemp("subsample")
    return dict(seqs=seqs, samples=samples, kept=kept, x=_write_cohort(str(root / "x"), samples), xk=_write_cohort(str(root / "xk"), kept), root=root)


def _dataset_outputs(ctx, seqs, paths, tmp, tag, subsample):
    ds = core.Dataset(ctx, NAMES, LENGTHS, seqs, core.default_params(min_coverage=2, calling_threshold=2))
    if subsample:
        ds.set_subsample(*subsample)
    ds.add_sample_bams(paths)
    ds.finalize()
    ds.coverage_run()
    ds.run()
    out = dict(stats=[ds.sample_stats(i).tolist() for i in range(len(paths))], acc=ds.coverage_accumulators().tolist())
    sites, smp = ds.results()
    out["sites"], out["site_samples"] = sites.tobytes(), smp.tobytes()
    files = []
    cp, ip = os.path.join(tmp, "called_" + tag), os.path.join(tmp, "indiv_" + tag)
    ds.write_calls(cp, ip)
    files += [open(cp, "rb").read(), open(ip, "rb").read()]
    for i in range(len(paths)):
        c = os.path.join(tmp, "cov%d_%s" % (i, tag))
        ds.write_coverage(i, c, c + ".detail")
        files += [open(c, "rb").read(), open(c + ".detail", "rb").read()]
    out["files"] = files
    ds.close()
    return out, len(sites)


@pytest.mark.parametrize("pack", [None, "host"])
def test_a_dataset_that_subsamples_equals_one_built_from_the_kept_reads(ctx, cohort, tmp_path, pack):
    with _env(MSNV_PACK=pack):
        a, n_sites = _dataset_outputs(ctx, cohort["seqs"], cohort["x"], str(tmp_path), "sub", (42, .25))
        b, _ = _dataset_outputs(ctx, cohort["seqs"], cohort["xk"], str(tmp_path), "kept", None)
        whole, n_whole = _dataset_outputs(ctx, cohort["seqs"], cohort["x"], str(tmp_path), "all", None)
    for k in ("stats", "acc", "sites", "site_samples", "files"):
        assert a[k] == b[k], k
    assert [s[0] for s in a["stats"]] == [64, 64, 64] and [s[0] for s in whole["stats"]] == [257, 257, 257]
    assert n_sites > 0 and a["files"][0] and a["files"] != whole["files"]      # (something is called, and the subsample is not the whole)
    # the other record entries take the same seam: one stream, many streams, streams in device memory
    with _env(MSNV_PACK=pack):
        for how in ("one", "many", "device"):
            ds = core.Dataset(ctx, NAMES, LENGTHS, cohort["seqs"])
            ds.set_subsample(42, .25)
            arrs = [np.frombuffer(s, np.uint8) for s in cohort["samples"]]
            if how == "one":
                for x in arrs:
                    ds.add_sample_records(x)
            elif how == "many":
                ds.add_samples_records(arrs)
            else:
                hip = C.CDLL("libamdhip64.so")
                ptrs = _on_device(hip, cohort["samples"])
                ds.add_samples_records_device(ptrs, [len(s) for s in cohort["samples"]])
                for p in ptrs:
                    hip.hipFree(C.c_void_p(p))
            assert [ds.sample_stats(i).tolist() for i in range(3)] == a["stats"], how
            ds.close()


def test_entries_that_cannot_subsample_refuse_and_leave_the_dataset_alone(ctx, cohort):
    hip = C.CDLL("libamdhip64.so")
    ds = core.Dataset(ctx, NAMES, LENGTHS, cohort["seqs"])
    ds.set_subsample(42, .25)
    before = ds.info()
    buf = C.c_void_p(); assert hip.hipMalloc(C.byref(buf), C.c_size_t(1 << 20)) == 0
    s0 = np.frombuffer(cohort["samples"][0], np.uint8)
    assert hip.hipMemcpy(buf, C.c_void_p(s0.ctypes.data), C.c_size_t(s0.size), 1) == 0
    calls = [lambda: ds.add_samples_records_resident(buf.value, 1 << 20, [0], [s0.size]),
             lambda: ds.deal_bams_device(cohort["x"], [0, 0], 1, buf.value, 1 << 20),
             lambda: ds.inflate_bams_device(cohort["x"], buf.value, 1 << 20)]
    for call in calls:
        with pytest.raises(_lib.MsnvError) as e:
            call()
        assert e.value.code == _lib.EINVAL and "subsample" in str(e.value)
        assert ds.info() == before
    ds.add_sample_bams(cohort["x"][:1])
    before = ds.info()
    with pytest.raises(_lib.MsnvError) as e:                       # once a sample is in, the setting stays
        ds.set_subsample(7, .5)
    assert e.value.code == _lib.EINVAL and ds.info() == before and ds.subsample == (42, .25)
    ds.close()
    hip.hipFree(buf)
    # the N-rank feed (metasnv_amd/parallel.py) refuses such a dataset before it reads a file
    from metasnv_amd import parallel
    ds = core.Dataset(ctx, NAMES, LENGTHS, cohort["seqs"])
    ds.set_subsample(42, .25)
    before = ds.info()
    with pytest.raises(ValueError):
        parallel.feed_sharded(ds, cohort["x"], [0, 0], read_records=lambda p: np.zeros(0, np.uint8))
    assert ds.info() == before
    ds.close()


def _qacompute(args):
    return subprocess.run([os.path.join(TOOLS, "msnv_qacompute")] + args, capture_output=True, text=True, timeout=300)


def test_the_drop_in_takes_dash_a(cohort, tmp_path):
    x, xk = cohort["x"][0], cohort["xk"][0]
    regions = str(tmp_path / "regions")
    open(regions, "w").write("ctgA 10 400 first\nctgB 1 300 second\nnowhere 1 5 none\n")
    for extra, suffixes in (([], ["", ".detail"]), (["-m", "-p", "50", "-x", regions], ["", ".detail", ".profile", ".specific"])):
        tag = "ex" if extra else "plain"
        a, b, c, d = (str(tmp_path / (n + tag)) for n in ("sub", "kept", "one", "all"))
        r = _qacompute(["-a", "42.25"] + extra + ["-d", "-i", x, a]); assert r.returncode == 0, r.stderr
        r = _qacompute(extra + ["-d", "-i", xk, b]); assert r.returncode == 0, r.stderr
        r = _qacompute(["-a", "1"] + extra + ["-d", "-i", x, c]); assert r.returncode == 0, r.stderr
        r = _qacompute(extra + ["-d", "-i", x, d]); assert r.returncode == 0, r.stderr
        for sfx in suffixes:
            assert open(a + sfx, "rb").read() == open(b + sfx, "rb").read(), (tag, sfx)
            assert open(c + sfx, "rb").read() == open(d + sfx, "rb").read(), (tag, sfx)      # -a 1: a fraction of 0, nothing is subsampled
        assert open(a, "rb").read() != open(d, "rb").read()
    out = str(tmp_path / "refused")
    for bad in (["-a", "-3.5"], ["-s", "100"], ["-h", regions]):
        r = _qacompute(bad + ["-d", "-i", x, out])
        assert r.returncode == 1 and not os.path.exists(out), bad


def _tree(root):
    out = {}
    for dp, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out


def test_the_launcher_subsamples_every_bam(cohort, tmp_path):
    """metaSNV.py --subsample 42.25 on X writes the project directory of the plain run on X'."""
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for n, s in zip(NAMES, cohort["seqs"]):
            f.write(">%s\n%s\n" % (n, s))
    # the BAMs' paths go into the project (all_samples, table columns): both runs read them from ONE place, filled twice
    import shutil
    bams = str(tmp_path / "bams")
    lst = str(tmp_path / "all_samples")
    trees = {}
    for tag, src, extra in (("sub", cohort["x"], ["--subsample", "42.25"]), ("kept", cohort["xk"], [])):
        shutil.rmtree(bams, ignore_errors=True); os.makedirs(bams)
        paths = [shutil.copy(p, os.path.join(bams, os.path.basename(p))) for p in src]
        open(lst, "w").write("\n".join(paths) + "\n")
        proj = str(tmp_path / tag / "proj")
        os.makedirs(os.path.dirname(proj))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "metaSNV.py"), proj, lst, fa, "--min_pos_cov", "2", "--min_pos_snvs", "2"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        trees[tag] = _tree(proj)
    assert sorted(trees["sub"]) == sorted(trees["kept"])
    for k in trees["sub"]:
        assert trees["sub"][k] == trees["kept"][k], k
    assert trees["sub"]["snpCaller/called_SNPs"].count(b"\n") > 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, "metaSNV.py"), str(tmp_path / "bad" / "proj"), lst, fa, "--subsample", "-3.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--subsample" in r.stderr
