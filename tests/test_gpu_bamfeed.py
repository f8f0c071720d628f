"""The BAM feed's host side (csrc/bamfeed.cpp: files read, BGZF blocks indexed, inflated on the device or the host, checked, handed on)
on the routes no other test takes: the staged form in several batches and with every batch on the host, msnv_bam_records_many,
msnv_dataset_inflate_bams_device called directly, and -- on every route -- an error that names the file it belongs to."""
import ctypes as C
import os

import numpy as np
import pytest

from metasnv_amd import core, _lib

pytestmark = pytest.mark.gpu


class _Workload:
    pass


@pytest.fixture(scope="module")
def wl(tmp_path_factory):
    """4 samples, 2 x 60 kb contigs, 16x, levels 6/1/0/9 (the workload of test_resident_device_inflate_checks_every_block_in_hbm), the host
    reader's record streams, and copies of the second file with flipped payload bits / a flipped bit of a trailer CRC in its third block."""
    d = tmp_path_factory.mktemp("bamfeed")
    w = _Workload()
    w.dir = d
    sp = core.synth_params(n_species=2, contig_len=60000, n_samples=4, mean_cov=16.0, frac_paired=0.3, snv_density=0.02, seed=13)
    w.syn = core.Synth(sp)
    w.fa = str(d / "ref.fa"); w.syn.write_fasta(w.fa)
    w.paths = []
    for i in range(sp.n_samples):
        p = str(d / ("s%d.bam" % i))
        core.write_bam(p, w.syn.names, w.syn.lengths, w.syn.sample_records(i), level=[6, 1, 0, 9][i]); w.paths.append(p)
    assert sum(os.path.getsize(p) for p in w.paths) > (2 << 20)
    w.records = [core.read_bam(p)["records"] for p in w.paths]
    raw = bytearray(open(w.paths[1], "rb").read())
    off = 0
    for _ in range(2):
        off += (raw[off + 16] | raw[off + 17] << 8) + 1
    bsize = (raw[off + 16] | raw[off + 17] << 8) + 1
    w.bad = {}
    for kind in ("payload", "crc"):
        bad = bytearray(raw)
        if kind == "crc":
            bad[off + bsize - 8] ^= 0x01
        else:
            for k in (40, 41, 90):
                bad[off + 18 + k] ^= 0x5a
        w.bad[kind] = str(d / ("bad_%s.bam" % kind)); open(w.bad[kind], "wb").write(bad)
    w.missing = str(d / "missing.bam")
    return w


def _calls(wl, ctx, tag):
    ds = core.Dataset.from_files(ctx, wl.paths[0], wl.fa)
    t0 = core.host_timers()
    ds.add_sample_bams(wl.paths, 3)
    t1 = core.host_timers()
    info = ds.finalize(); ds.run()
    c, i = str(wl.dir / ("c_" + tag)), str(wl.dir / ("i_" + tag))
    ds.write_calls(c, i, None, None)
    ds.close()
    return open(c, "rb").read(), open(i, "rb").read(), info["n_pileup_bases"], {k: t1[k] - t0[k] for k in t0}


def test_staged_form_in_several_batches_equals_the_host_inflate(wl, monkeypatch):
    """MSNV_PACK=host, MSNV_INFLATE=device, 1 MB batches (the files hold more than 2 MB: several batches through the pinned staging), and the
    same with MSNV_TEST_NO_STAGING=1 (every batch a host batch): the bytes of called_SNPs / indiv_called and the pileup bases of MSNV_INFLATE=host."""
    monkeypatch.setenv("MSNV_PACK", "host")
    ctx = core.Context(0)
    monkeypatch.setenv("MSNV_INFLATE", "host")
    want = _calls(wl, ctx, "host")
    assert want[0].count(b"\n") > 10 and want[2] > 0 and want[3]["inflate_device_wall_s"] == 0.0
    monkeypatch.setenv("MSNV_INFLATE", "device"); monkeypatch.setenv("MSNV_INFLATE_BATCH_MB", "1")
    got = _calls(wl, ctx, "staged")
    assert got[:3] == want[:3] and got[3]["inflate_device_wall_s"] > 0.0
    monkeypatch.setenv("MSNV_TEST_NO_STAGING", "1")
    got = _calls(wl, ctx, "nostaging")
    assert got[:3] == want[:3] and got[3]["inflate_device_wall_s"] == 0.0 and got[3]["inflate_host_s"] > 0.0
    ctx.close()


@pytest.mark.parametrize("batch_mb", ["1", None])
def test_read_bam_records_through_the_device_inflate(wl, monkeypatch, batch_mb):
    """msnv_bam_records_many with a context and MSNV_INFLATE=device, in batches of 1 MB and of the default size: every stream is the host reader's."""
    monkeypatch.setenv("MSNV_INFLATE", "device")
    if batch_mb:
        monkeypatch.setenv("MSNV_INFLATE_BATCH_MB", batch_mb)
    ctx = core.Context(0)
    t0 = core.host_timers()
    got = core.read_bam_records(wl.paths, ctx, 3)
    assert core.host_timers()["inflate_device_wall_s"] > t0["inflate_device_wall_s"]
    assert len(got) == len(wl.records)
    for g, w in zip(got, wl.records):
        assert g.size == w.size and g.tobytes() == w.tobytes()
    ctx.close()


def test_inflate_bams_device_called_directly(wl, monkeypatch):
    """msnv_dataset_inflate_bams_device: sizes, 16-aligned offsets with at least 16 bytes behind every stream, the bytes in the device buffer,
    qaCompute's statistics and the aligned bases per contig against the host route; an output one byte short is MSNV_ECAPACITY, files of more
    than one batch MSNV_EDOMAIN."""
    hip = C.CDLL("libamdhip64.so")
    ctx = core.Context(0)
    ds = core.Dataset.from_files(ctx, wl.paths[0], wl.fa)
    nc, n = len(wl.syn.names), len(wl.paths)
    sizes = [int(r.size) for r in wl.records]
    need, o = 0, 0
    for s in sizes:                                              # (what the entry point asks for: 32 bytes behind the last stream it writes)
        need = o + s + 32
        o += (s + 31) & ~15
    d = C.c_void_p(); assert hip.hipMalloc(C.byref(d), C.c_size_t(need + 64)) == 0
    cb = np.zeros(nc, np.uint64)
    t0 = core.host_timers()
    offs, got_sizes, stats = ds.inflate_bams_device(wl.paths, d.value, need, contig_bases=cb, host_threads=3)
    assert core.host_timers()["inflate_host_s"] == t0["inflate_host_s"]       # no block went through the host decoder
    assert [int(x) for x in got_sizes] == sizes
    assert all(int(x) % 16 == 0 for x in offs) and int(offs[0]) == 0
    for i in range(n):
        end = int(offs[i + 1]) if i + 1 < n else need
        assert end - (int(offs[i]) + sizes[i]) >= 16, i
    got = np.zeros(need, np.uint8); assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), d, C.c_size_t(need), 2) == 0
    for i in range(n):
        assert got[int(offs[i]):int(offs[i]) + sizes[i]].tobytes() == wl.records[i].tobytes(), i
    nobody = np.full(nc, -1, np.int32)
    want_cb = np.zeros(nc, np.uint64)
    want_stats = []
    for r in wl.records:
        want_stats.append(core.partition_records(r, nobody, 1)[1]); core.contig_bases(r, nc, into=want_cb)
    assert np.array_equal(stats, np.stack(want_stats)) and np.array_equal(cb, want_cb) and int(cb.sum()) > 0
    with pytest.raises(_lib.MsnvError) as e:
        ds.inflate_bams_device(wl.paths, d.value, need - 1, host_threads=3)
    assert e.value.code == _lib.ECAPACITY
    monkeypatch.setenv("MSNV_INFLATE_BATCH_MB", "1")
    with pytest.raises(_lib.MsnvError) as e:
        ds.inflate_bams_device(wl.paths, d.value, need, host_threads=3)
    assert e.value.code == _lib.EDOMAIN
    hip.hipFree(d); ds.close(); ctx.close()


_ROUTES = ["staged", "staged-without-staging", "resident", "read_bams"]


def _feed(route, wl, ctx, paths, monkeypatch):
    monkeypatch.setenv("MSNV_INFLATE", "device")
    if route == "read_bams":
        return core.read_bam_records(paths, ctx, 3)
    monkeypatch.setenv("MSNV_PACK", "device" if route == "resident" else "host")
    if route == "staged-without-staging":
        monkeypatch.setenv("MSNV_TEST_NO_STAGING", "1")
    ds = core.Dataset.from_files(ctx, wl.paths[0], wl.fa)
    try:
        ds.add_sample_bams(paths, 3)
    finally:
        ds.close()


def _names_only(msg, bad, others):
    return os.path.basename(bad) in msg and not any(os.path.basename(p) in msg for p in others)


@pytest.mark.parametrize("kind", ["payload", "crc"])
@pytest.mark.parametrize("route", _ROUTES)
def test_a_corrupted_file_is_the_one_the_error_names(wl, monkeypatch, route, kind):
    """Three files, the middle one with flipped payload bits / a flipped bit of a trailer CRC: MSNV_EFORMAT, and the message holds that file's
    name and neither of the others'."""
    ctx = core.Context(0)
    with pytest.raises(_lib.MsnvError) as e:
        _feed(route, wl, ctx, [wl.paths[0], wl.bad[kind], wl.paths[2]], monkeypatch)
    ctx.close()
    assert e.value.code == _lib.EFORMAT
    assert _names_only(str(e.value), wl.bad[kind], [wl.paths[0], wl.paths[2]]), str(e.value)


@pytest.mark.parametrize("route", _ROUTES + ["deal_bams_device"])
def test_a_missing_file_is_the_one_the_error_names(wl, monkeypatch, route):
    """Three files, the middle one absent: MSNV_EIO with that file's name."""
    paths = [wl.paths[0], wl.missing, wl.paths[2]]
    ctx = core.Context(0)
    with pytest.raises(_lib.MsnvError) as e:
        if route == "deal_bams_device":
            ds = core.Dataset.from_files(ctx, wl.paths[0], wl.fa)
            try:
                ds.deal_bams_device(paths, np.zeros(len(wl.syn.names), np.int32), 1, 0, 0, host_threads=3)      # (refused before the output is looked at)
            finally:
                ds.close()
        else:
            _feed(route, wl, ctx, paths, monkeypatch)
    ctx.close()
    assert e.value.code == _lib.EIO
    assert _names_only(str(e.value), wl.missing, [wl.paths[0], wl.paths[2]]), str(e.value)
