"""What the tests of the per-read stage share: one dataset built by the host stage (csrc/pack.cpp, MSNV_PACK=host) and by the device
stage (csrc/devpack.hip) from the same record streams, compared column by column, summary by summary and call by call -- and against
the oracle's text (tests/test_gpu_devpack.py, tests/test_gpu_record_walk.py)."""
import ctypes as C
import os

import numpy as np

import bamtools as bt
from metasnv_amd import core
from parity import run_oracle, first_diff

COLUMNS = ["hdr", "hdr4", "hdr8m", "blk", "seq", "qual", "s_read_base", "s_seq_base", "ref4", "pairs", "work", "chunks", "cov_iv", "cov_pairs", "cov_work",
           # the rest of what finalize uploads (csrc/finalize.cpp; a table the layout does not allocate holds 0 bytes)
           "ref_lc", "tile_vbeg", "tile_vend", "tile_nslots", "active_tiles", "gather_tiles", "tile_slot_start", "tile_slot_u16", "tile_slot_wide", "slot_off",
           "gate_tiles", "gate_tiles_dense", "gate_tiles_staged", "tile_stage_idx", "merged_groups", "tile_pair_start", "tile_pair_merged",
           "s_cov_base", "tile_len", "tile_contig_dev"]


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _build(where, names, lengths, seqs, samples, bed=None, params=None, many=False, device_ptrs=False, finalize=None):
    with _env(MSNV_PACK=where, MSNV_FINALIZE=finalize):
        ctx = core.Context(0)
        ds = core.Dataset(ctx, names, lengths, seqs, params)
        if bed:
            ds.set_bed(bed)
        if device_ptrs:
            # record streams already in HBM (what an all-to-all over RCCL leaves there): plain hipMalloc + hipMemcpy through the
            # runtime the library itself is linked to -- torch in this process would bring a second HIP runtime
            hip = C.CDLL("libamdhip64.so")
            ptrs, sizes = [], []
            for smp in samples:
                a = np.ascontiguousarray(smp, dtype=np.uint8)
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), C.c_size_t(max(1, a.size))) == 0
                if a.size:
                    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.size), 1) == 0
                ptrs.append(p.value); sizes.append(a.size)
            ds.add_samples_records_device(ptrs, sizes)
            for p in ptrs:
                hip.hipFree(C.c_void_p(p))
        elif many:
            ds.add_samples_records(samples)
        else:
            for s in samples:
                ds.add_sample_records(s)
        info = ds.finalize()
    return ctx, ds, info


def _same_dataset(names, lengths, seqs, samples, bed=None, params=None, many=False, device_ptrs=False, check_oracle=True, finalize=None, stats=None):
    """stats: a dict that receives the device-packed dataset's pack_stats() (which route its per-read stage took).
    finalize: None = the tile index of the device-packed dataset is built in HBM where it can be (devfin_*), "host" = its headers come
    down and the host loops of finalize_dataset (csrc/finalize.cpp) build it."""
    ch, dh, ih = _build("host", names, lengths, seqs, samples, bed, params)
    cd, dd, idv = _build("device", names, lengths, seqs, samples, bed, params, many=many, device_ptrs=device_ptrs, finalize=finalize)
    try:
        if stats is not None:
            stats.update(dd.pack_stats())
        for k in ("n_reads", "n_reads_pileup", "n_pileup_bases", "bytes_headers", "bytes_cigar", "bytes_seq", "bytes_qual", "n_tiles", "n_pairs", "n_work",
                  "allele_planes", "sampled_mismatch_ppm"):
            assert ih[k] == idv[k], (k, ih[k], idv[k])
        for col in COLUMNS:
            a, b = dh.column(col), dd.column(col)
            assert a.size == b.size, (col, a.size, b.size)
            if not np.array_equal(a, b):
                i = int(np.flatnonzero(a != b)[0])
                raise AssertionError("column %s differs at byte %d of %d: host %s device %s" % (col, i, a.size, a[max(0, i - 4):i + 12].tolist(), b[max(0, i - 4):i + 12].tolist()))
        for s in range(len(samples)):
            assert np.array_equal(dh.sample_stats(s), dd.sample_stats(s)), s
        assert dh.first_line() == dd.first_line()
        if not bed:                                               # (the per-contig first lines are defined for a whole-BAM dataset only)
            fa, fb = dh.first_lines(), dd.first_lines()
            assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
        dd.run(); dh.run()
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            out = []
            for tag, ds in (("h", dh), ("d", dd)):
                pp, ip = os.path.join(td, "c" + tag), os.path.join(td, "i" + tag)
                ds.write_calls(pp, ip)
                out.append((open(pp).read(), open(ip).read()))
        assert out[0] == out[1]
        if check_oracle:
            orac = run_oracle(names, lengths, seqs, samples, bed=bed, params=params)
            assert out[1][0] == orac[0], first_diff(out[1][0], orac[0])
            assert out[1][1] == orac[1], first_diff(out[1][1], orac[1])
        return idv
    finally:
        dh.close(); dd.close(); ch.close(); cd.close()


def _decoy_stream():
    """40 records of 50 bases on a 6000-base contig; every third carries, in an aux field, the bytes of plausible record headers 40 bytes
    apart: a walk that enters there on a guess ends cleanly at the wrong place, and only the seam check can tell.  Returns (ref, stream)."""
    import struct
    ref = "ACGT" * 1500

    def fake(nxt):                      # 36 header bytes of a "record" with block_size nxt - 4 whose fields pass every plausibility test (name: 2 bytes, NUL-terminated)
        return struct.pack("<iiiBBHHHiiii", nxt - 4, 0, 5, 2, 60, 4680, 0, 0, 0, -1, -1, 0)
    decoy = (fake(40) + b"a\0\0\0") * 6
    recs = []
    for k in range(40):
        recs.append(bt.make_record(0, 10 + 20 * k, "50M", ref[10 + 20 * k:60 + 20 * k], name="r%d" % k, aux=b"ZZZ" + decoy[:200] if k % 3 == 0 else b""))
    return ref, bt.records(*recs)
