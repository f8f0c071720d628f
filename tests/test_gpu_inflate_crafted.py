"""The device DEFLATE decoder (csrc/inflate_k.hip: msnv_inflate_blocks) on the hand-assembled streams of tests/deflate_craft.py, judged by
zlib and not by the host decoder it shares its design with: every valid stream is inflated ON THE DEVICE to zlib's bytes (the kernel's
table caps are zlib's bounds, so it may refuse none), every malformed one ends as MSNV_EFORMAT.  And msnv_crc_blocks, which the resident
route checks every member with, at the member sizes where its lane count and the tail behind its 4-byte loop change."""
import os

import pytest

import deflate_craft as dc
from metasnv_amd import core, _lib

pytestmark = pytest.mark.gpu


def test_device_inflates_every_valid_crafted_stream(tmp_path, monkeypatch):
    """All valid cases in ONE file = one launch of a thousand wavefronts: zlib's bytes, nothing handed to the host decoder; the payloads
    of the window families start at all four byte alignments (tests/test_deflate_crafted.py checks the file for that).  MSNV_INFLATE_CHECK=1:
    every block also against the CRC-32 of its trailer."""
    data, want = dc.valid_file()
    p = str(tmp_path / "valid.gz")
    open(p, "wb").write(data)
    cases = dc.valid_cases()
    ctx = core.Context(0)
    for check in ("0", "1"):
        monkeypatch.setenv("MSNV_INFLATE_CHECK", check)
        dev, cnt = core.bgzf_inflate(p, ctx)
        got = dev.tobytes()
        if got != want:                                            # name the first case that differs
            o = 0
            for c in cases:
                assert got[o:o + len(c.intended)] == c.intended, c.name
                o += len(c.intended)
        assert got == want
        assert cnt["host_blocks"] == 0 and cnt["blocks"] == sum(1 for c in cases if c.intended) and cnt["bytes"] == len(want)
    ctx.close()


def test_malformed_crafted_streams_are_format_errors(tmp_path):
    """A file that mixes malformed members with valid ones is MSNV_EFORMAT; then every malformed case in a file of its own (between two
    valid members): zlib refuses each, so the device route must (the kernel may refuse early and let the host decoder word the error)."""
    good = [c for c in dc.valid_cases() if c.family in ("every_symbol", "literal_batching")]
    bad = dc.malformed_cases()
    ctx = core.Context(0)
    mixed, k = [], 0
    for c in bad:
        mixed += [(good[k % len(good)].stream, good[k % len(good)].intended), (c.stream, c.intended)]; k += 1
    p = str(tmp_path / "mixed.gz")
    open(p, "wb").write(dc.bgzf(mixed))
    with pytest.raises(_lib.MsnvError) as e:
        core.bgzf_inflate(p, ctx)
    assert e.value.code == _lib.EFORMAT
    for c in bad:
        q = str(tmp_path / "bad.gz")
        open(q, "wb").write(dc.bgzf([(good[0].stream, good[0].intended), (c.stream, c.intended), (good[1].stream, good[1].intended)]))
        with pytest.raises(_lib.MsnvError) as e:
            core.bgzf_inflate(q, ctx)
        assert e.value.code == _lib.EFORMAT, c.name
    # and the valid members of those files alone are fine (the errors above are the malformed members')
    q = str(tmp_path / "good.gz")
    open(q, "wb").write(dc.bgzf([(g.stream, g.intended) for g in good]))
    dev, cnt = core.bgzf_inflate(q, ctx)
    assert dev.tobytes() == b"".join(g.intended for g in good) and cnt["host_blocks"] == 0
    ctx.close()


CRC_SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 65280, 65536]


def test_crc_kernel_at_the_member_sizes_where_its_lanes_change(tmp_path, monkeypatch):
    """msnv_crc_blocks gives lane l bytes [1024 l, 1024 l + 1024) of a member, four at a time and a tail of 0-3: members of 1 .. 5, 1024 +- 1,
    2048 +- 1, 65280 and 65536 bytes are 1, 2, 3 and 64 lanes and every tail.  A BAM with such members through the resident route (device
    inflate + device pack) gives the oracle's calls; one flipped bit in the trailer CRC of each of those members is MSNV_EFORMAT, and
    passes with MSNV_INFLATE_CHECK=0."""
    import bamtools as bt
    from parity import run_oracle
    monkeypatch.setenv("MSNV_INFLATE", "device"); monkeypatch.setenv("MSNV_PACK", "device")
    sp = core.synth_params(n_species=2, contig_len=30000, n_samples=2, mean_cov=12.0, frac_paired=0.3, snv_density=0.02, seed=21)
    syn = core.Synth(sp)
    fa = str(tmp_path / "ref.fa"); syn.write_fasta(fa)
    recs = [syn.sample_records(i) for i in range(sp.n_samples)]
    paths = [str(tmp_path / ("m%d.bam" % i)) for i in range(sp.n_samples)]
    members = bt.write_bam_members(paths[0], syn.names, syn.lengths, recs[0].tobytes(), CRC_SIZES)
    bt.write_bam_members(paths[1], syn.names, syn.lengths, recs[1].tobytes(), CRC_SIZES[::-1])
    assert [m[2] for m in members[:len(CRC_SIZES)]] == CRC_SIZES
    want = run_oracle(syn.names, syn.lengths, syn.seqs, recs)
    ctx = core.Context(0)
    t0 = core.host_timers()
    ds = core.Dataset.from_files(ctx, paths[0], fa)
    ds.add_sample_bams(paths, 2)
    info = ds.finalize(); ds.run()
    ds.write_calls(str(tmp_path / "c"), str(tmp_path / "i"), None, None)
    assert core.host_timers()["inflate_host_s"] == t0["inflate_host_s"]          # no member went to the host decoder
    assert open(tmp_path / "c").read() == want[0] and open(tmp_path / "i").read() == want[1] and want[0].count("\n") > 10
    assert info["n_pileup_bases"] == want[3]
    ds.close()
    raw = open(paths[0], "rb").read()
    badp = str(tmp_path / "bad_crc.bam")
    for (off, bsize, n), bit in zip(members[:len(CRC_SIZES)], range(len(CRC_SIZES))):
        bad = bytearray(raw)
        bad[off + bsize - 8 + bit % 4] ^= 1 << (bit % 8)
        open(badp, "wb").write(bad)
        monkeypatch.setenv("MSNV_INFLATE_CHECK", "1")
        ds = core.Dataset.from_files(ctx, paths[1], fa)
        with pytest.raises(_lib.MsnvError) as e:
            ds.add_sample_bams([paths[1], badp], 2)
        assert e.value.code == _lib.EFORMAT, n
        ds.close()
        monkeypatch.setenv("MSNV_INFLATE_CHECK", "0")
        ds = core.Dataset.from_files(ctx, paths[1], fa)
        ds.add_sample_bams([paths[1], badp], 2)
        assert ds.finalize()["n_pileup_bases"] == info["n_pileup_bases"], n
        ds.close()
    ctx.close()
