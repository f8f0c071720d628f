"""`samtools mpileup -a / -aa`, `-s` and `-O` (msnv_mpileup_text_opts; csrc/mptext.cpp + csrc/mptext_k.hip; tools/msnv_mpileup): a
line for every position, a MAPQ column and a read-offset column, formatted on the device.

The oracle (oracle/orc_mpileup.c) knows none of the three, so the expected text is the oracle's text plus what tests/mpcolsmodel.py
derives -- the two columns from a plain pileup of unpaired reads, the zero-depth lines by the rule of include/msnv.h -- and the
comparison stays BYTE FOR BYTE.  tests/test_mpcols_model.py pins that model on the oracle without a device.  With pairs in a cohort
the model does not apply (it has no mates edit): there the extra columns are stripped and what is left must be the oracle's text."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import orc
from bamtools import make_record as R, records
from metasnv_amd import core, _lib
from mpcolsmodel import add_columns, columns, fill_all, pushed_tids, strip_columns
from parity import synth_case, first_diff
from test_mpcols_model import random_cohort

pytestmark = pytest.mark.gpu
T, B = core.mpileup_text_geometry()          # positions per tile, read descriptors per LDS batch (csrc/mptext.h)
TOOLS = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools")
EMPTY = np.zeros(0, np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def ref_of(n, seed=1):
    rnd = random.Random(seed)
    return "".join(rnd.choice("ACGT") for _ in range(n))


def expect(names, lengths, seqs, samples, bed=None, level=0, mq=False, bp=False, **mp):
    """The oracle's text, the columns of the model behind its cells, the zero-depth lines of the model between its lines."""
    text = orc.mpileup_text(names, lengths, seqs, samples, bed=bed, mp=mp)
    filt = dict(bed=bed, flag_filter=mp.get("flag_filter", 0x704), min_mapq=mp.get("min_mapq", 0), count_orphans=mp.get("count_orphans", 0))
    if level:
        # fill_all takes "has a line" for "in play"; the BED overlap filter is read-level, so: every contig with a pushed read has a line
        tid_of = {n: i for i, n in enumerate(names)}
        assert pushed_tids(names, seqs, samples, **filt) <= {tid_of[ln.split("\t", 1)[0]] for ln in text.split("\n")[:-1]}
    if mq or bp:
        text = add_columns(text, names, columns(names, lengths, seqs, samples, mp.get("min_baseq", 13), **filt), mq, bp)
    if level:
        text = fill_all(text, names, lengths, seqs, bed, len(samples), int(mq) + int(bp), level)
    return text.encode("latin-1")


def check(ctx, names, lengths, seqs, samples, bed=None, level=0, mq=False, bp=False, **mp):
    want = expect(names, lengths, seqs, samples, bed, level, mq, bp, **mp)
    got = ctx.mpileup_text(names, lengths, seqs, samples, bed=bed, all_positions=level, output_mq=mq, output_bp=bp, **mp)
    assert got == want, first_diff(got.decode("latin-1"), want.decode("latin-1"))
    st = ctx.mpileup_stats
    assert st["text_bytes"] == len(got) and st["lines"] == got.count(b"\n") and st["samples"] == len(samples)
    return got


# ------------------------------------------------------------------------------------------------ 1. literals
def test_literal_all_three_options(ctx):
    got = ctx.mpileup_text(["c"], [8], ["ACGTACGT"], [records(R(0, 2, "2M", "GT", [30, 30], mapq=60))], all_positions=1, output_mq=True, output_bp=True)
    z = "\t0\t*\t*\t*\t*\n"
    want = "c\t1\tA" + z + "c\t2\tC" + z + "c\t3\tG\t1\t^].\t?\t]\t1\n" + "c\t4\tT\t1\t.$\t?\t]\t2\n" + "c\t5\tA" + z + "c\t6\tC" + z + "c\t7\tG" + z + "c\t8\tT" + z
    assert got.decode() == want


def test_literal_offsets_over_a_deletion(ctx):
    got = ctx.mpileup_text(["c"], [8], ["ACGTACGT"], [records(R(0, 0, "2M1D2M", "ACTA", [30] * 4, mapq=0))], output_bp=True).decode()
    assert [ln.split("\t")[6] for ln in got.split("\n")[:-1]] == ["1", "2", "3", "3", "4"]
    assert got.split("\n")[2] == "c\t3\tG\t1\t*\t?\t3"
    got = ctx.mpileup_text(["c"], [8], ["ACGTACGT"], [records(R(0, 0, "2M1D2M", "ACTA", [30] * 4, mapq=0))], output_mq=True).decode()
    assert [ln.split("\t")[6] for ln in got.split("\n")[:-1]] == ["!"] * 5


def test_option_values_are_checked(ctx):
    for bad in (dict(all_positions=3), dict(all_positions=-1)):
        with pytest.raises(_lib.MsnvError) as e:
            ctx.mpileup_text(["c"], [8], ["ACGTACGT"], [EMPTY], **bad)
        assert e.value.code == _lib.EINVAL
    with pytest.raises(AttributeError):                             # the options are keywords of their own, everything else is msnv_params
        ctx.mpileup_text(["c"], [8], ["ACGTACGT"], [EMPTY], output_qname=True)


# ------------------------------------------------------------------------------------------------ 2. off means off
def _records_call(ctx, fn, opts, syn, samples):
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
    text, nb, st = C.POINTER(C.c_char)(), C.c_uint64(), (C.c_uint64 * 8)()
    head = [ctx._h, C.byref(rd), C.byref(p)] + ([opts] if fn.endswith("_ex") else [])
    _lib.check(getattr(_lib.lib, fn)(*head, 0, None, None, None, ptrs, sizes, len(bufs), C.byref(text), C.byref(nb), st))
    try:
        return C.string_at(text, nb.value)
    finally:
        _lib.lib.msnv_free(text)


def test_off_means_off(ctx):
    syn, samples = synth_case(n_species=2, contig_len=1500, n_samples=3, mean_cov=6.0, read_len=75, snv_density=0.02, frac_indel_reads=0.1, frac_clip_reads=0.1, seed=9)
    old = _records_call(ctx, "msnv_mpileup_text_records", None, syn, samples)
    assert old.count(b"\n") > 2000
    o = _lib.MpileupTextOpts(7, 7, 7, 7)
    _lib.lib.msnv_mpileup_text_opts_default(C.byref(o))
    assert (o.all_positions, o.output_mq, o.output_bp, o.reserved) == (0, 0, 0, 0)
    assert _records_call(ctx, "msnv_mpileup_text_records_ex", C.byref(o), syn, samples) == old
    assert _records_call(ctx, "msnv_mpileup_text_records_ex", None, syn, samples) == old
    o.reserved = 1
    with pytest.raises(_lib.MsnvError) as e:
        _records_call(ctx, "msnv_mpileup_text_records_ex", C.byref(o), syn, samples)
    assert e.value.code == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ 3. the columns do not disturb the text
def test_columns_do_not_disturb_the_text(ctx):
    rnd = random.Random(31)
    n_cells = 0
    for case in range(6):
        kw = dict(n_species=rnd.choice([1, 2]), contig_len=rnd.choice([300, 1500, 2049]), n_samples=rnd.choice([1, 3, 7]), mean_cov=rnd.choice([2, 8, 20]),
                  read_len=rnd.choice([36, 75, 100]), snv_density=0.02, error_rate=0.01, frac_lowq=0.2, frac_indel_reads=0.3, frac_clip_reads=0.1, frac_flagged=0.03,
                  lowercase_ref=1, frac_paired=rnd.choice([0.5, 1.0]), frac_noseq=0.03, seed=rnd.randrange(1 << 30))
        syn, samples = synth_case(**kw)
        mp = dict(ignore_overlaps=1, min_baseq=rnd.choice([0, 13, 30]))
        want = orc.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, mp=mp)
        got = ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, output_mq=True, output_bp=True, **mp).decode("latin-1")
        back, taken = strip_columns(got, 2)
        assert back == want, (case, first_diff(back, want))
        n_cells += len(taken)
        for _, _, cnt, quals, (mq, bp) in taken:
            assert len(mq) == len(quals)
            assert bp == "*" if cnt == 0 else len(bp.split(",")) == cnt
    assert n_cells > 5000


# ------------------------------------------------------------------------------------------------ 4. the values of the columns
@pytest.mark.parametrize("mq,bp", [(True, False), (False, True), (True, True)])
def test_column_values_on_random_unpaired_cohorts(ctx, mq, bp):
    rnd = random.Random(4100 + 2 * mq + bp)
    for case in range(25):
        names, lengths, seqs, samples = random_cohort(rnd)
        check(ctx, names, lengths, seqs if case % 5 else None, samples, mq=mq, bp=bp, min_baseq=rnd.choice([0, 13, 13, 31]), flag_filter=rnd.choice([0x704, 0]))


def test_mapq_characters_and_the_digits_of_an_offset(ctx):
    """MAPQ 0, 92, 93, 94 and 255; a read of 1100 bases (qpos + 1 crosses 9 -> 10, 99 -> 100, 999 -> 1000), one of them behind a soft
    clip and an insertion; a read without SEQ; -Q 0 and a -Q that empties cells."""
    ref = ref_of(1300)
    qual = [(i * 7) % 41 for i in range(1100)]
    recs = [R(0, 3, "1100M", ref[3:1103], qual, mapq=0, name="long"),
            R(0, 3, "7S990M3I100M", "A" * 7 + ref[3:993] + "TTT" + ref[993:1093], qual, mapq=92, flag=16, name="clip_ins"),
            R(0, 5, "4M1D3M", "*", name="noseq", mapq=93),
            R(0, 6, "8M2N990M", ref[6:14] + ref[16:1006], [20] * 998, mapq=94, name="skip"),
            R(0, 7, "3M", "ACG", [1, 40, 1], mapq=255, name="short")]
    for q in (0, 13, 30):
        text = check(ctx, ["c"], [1300], [ref], [records(*recs)], mq=True, bp=True, min_baseq=q)
    assert b"\t0\t*\t*\t*\t*\n" in text                                    # -Q 30 leaves cells without an element
    text = check(ctx, ["c"], [1300], [ref], [records(*recs)], mq=True, bp=True, min_baseq=0).decode()
    line = text.split("\n")[6].split("\t")                                   # position 10: all five reads, the SEQ-less one on its deletion
    assert line[1] == "10" and line[3] == "5" and line[6] == "!}~~~" and line[7] == "7,14,5,4,3"
    assert "\t999,1009," in text and "\t1000,1010," in text and "\t9,16," in text and "\t10,17," in text and "\t99,106," in text and "\t100,107," in text


# ------------------------------------------------------------------------------------------------ 5. sizes where the forms change
@pytest.mark.parametrize("n", [B - 1, B, B + 1, 2 * B + 1])
def test_reads_over_one_position_around_the_lds_batch(ctx, n):
    ref = ref_of(400, 2)
    rnd = random.Random(n)
    recs = sorted(((rnd.randrange(30, 50), i) for i in range(n)))
    recs = [R(0, p, "%dS%dM" % (i % 13 + 1, 60 - p), "A" * (i % 13 + 1) + ref[p:60], [rnd.randrange(10, 41) for _ in range(60 - p + i % 13 + 1)], name="r%d" % i,
              flag=16 * (i % 2), mapq=(i * 5) % 256) for p, i in recs]
    text = check(ctx, ["c"], [400], [ref], [records(*recs)], mq=True, bp=True)
    assert text.split(b"\n")[25].split(b"\t")[1] == b"56"
    check(ctx, ["c"], [400], [ref], [records(*recs), EMPTY, records(*recs[::2])], level=1, mq=True, bp=True)


def test_a_deletion_on_a_tile_edge(ctx):
    ref = ref_of(3 * T, 3)
    recs = [R(0, T - 3, "3M4D3M", ref[T - 3:T] + ref[T + 4:T + 7], name="over_the_edge", mapq=7),
            R(0, T - 2, "2M3D4M", ref[T - 2:T] + ref[T + 3:T + 7], name="first_star_on_tile_start", flag=16, mapq=8),
            R(0, 2 * T - 1, "1M2N2M", "ACG", name="skip_from_the_last_position", mapq=9)]
    for level in (0, 1):
        check(ctx, ["c"], [3 * T], [ref], [records(*recs)], level=level, mq=True, bp=True)


@pytest.mark.parametrize("length", [T - 1, T, T + 1, 3 * T + 5])
def test_the_stretch_behind_the_last_read(ctx, length):
    ref = ref_of(length, 4)
    text = check(ctx, ["c"], [length], [ref], [records(R(0, 2, "3M", ref[2:5]))], level=1)
    assert text.count(b"\n") == length
    text = check(ctx, ["c"], [length], [ref], [records(R(0, length - 2, "5M", ref[length - 2:] + "ACG"))], level=1, mq=True)      # a read over the contig's end
    assert text.count(b"\n") == length + 3


def test_empty_tiles_before_between_and_behind_the_reads(ctx):
    length = 6 * T + 7
    ref = ref_of(length, 5)
    a = records(R(0, 2 * T + 3, "10M", ref[2 * T + 3:2 * T + 13]), R(0, 4 * T + 10, "5M", ref[4 * T + 10:4 * T + 15], [2] * 5))
    b = records(R(0, 4 * T + 12, "5M", ref[4 * T + 12:4 * T + 17]))
    for kw in (dict(), dict(mq=True, bp=True)):
        text = check(ctx, ["c"], [length], [ref], [a, b], level=1, **kw)
        assert text.count(b"\n") == length
    check(ctx, ["c"], [length], [ref[:3 * T + 1]], [a, b], level=1)           # N beyond the FASTA's length
    check(ctx, ["c"], [length], None, [a, b], level=1)                        # no reference at all


def test_contigs_of_length_one(ctx):
    assert check(ctx, ["c", "d"], [1, 1], ["A", "C"], [records(R(0, 0, "1M", "A"))], level=1, bp=True) == b"c\t1\tA\t1\t^].$\tI\t1\n"
    assert check(ctx, ["c", "d"], [1, 1], ["A", "C"], [records(R(0, 0, "1M", "A"))], level=2) == b"c\t1\tA\t1\t^].$\tI\nd\t1\tC\t0\t*\t*\n"
    assert check(ctx, ["c", "d"], [1, 1], ["A", "C"], [records(R(1, 0, "1M", "A", [3]))], level=1) == b"d\t1\tC\t0\t*\t*\n"


def test_a_bed_region_that_starts_and_ends_inside_tiles(ctx):
    length = 5 * T
    ref = ref_of(length, 6)
    a = records(R(0, T, "10M", ref[T:T + 10], name="ends_on_the_region_start"), R(0, 2 * T + 3, "10M", ref[2 * T + 3:2 * T + 13]),
                R(0, 4 * T - 12, "10M", ref[4 * T - 12:4 * T - 2], name="over_the_region_end"), R(1, 5, "4M", "ACGT"))
    names, lengths, seqs = ["c", "d", "e"], [length, 40, 30], [ref, ref[:40], ref[:30]]
    for level in (1, 2):
        text = check(ctx, names, lengths, seqs, [a], bed=[(0, T + 5, 4 * T - 9), (2, 3, 1000)], level=level)
        assert text.startswith(b"c\t%d\t" % (T + 6)) and b"c\t%d\t" % (4 * T - 9) in text and b"c\t%d\t" % (4 * T - 8) not in text and b"d\t" not in text
        assert (b"e\t4\t" in text) == (level == 2) and b"e\t3\t" not in text and b"e\t31\t" not in text
    check(ctx, names, lengths, seqs, [a], bed=[(1, 0, 40)], level=1, mq=True)


def test_every_contig_of_the_header(ctx):
    """-aa: read-less contigs before, between and behind the contigs with reads, one of them without a FASTA record, one whose FASTA is
    shorter than its length; -a prints the contigs with reads only."""
    names = ["e0", "c1", "e2", "c3", "e4", "e5"]
    lengths = [T + 3, 2 * T, 1, 3 * T + 1, 2 * T - 1, 5]
    seqs = [ref_of(T + 3, 7), ref_of(2 * T, 8), "g", ref_of(2 * T, 9), None, "AC"]
    a = records(R(1, T - 2, "4M", seqs[1][T - 2:T + 2]), R(3, 5, "3M", seqs[3][5:8]))
    b = records(R(3, 2 * T - 4, "3M3D2M", "ACGTA", mapq=3))
    for level, n in ((1, lengths[1] + lengths[3]), (2, sum(lengths))):
        for kw in (dict(), dict(mq=True, bp=True)):
            assert check(ctx, names, lengths, seqs, [a, b], level=level, **kw).count(b"\n") == n
    text = check(ctx, names, lengths, seqs, [EMPTY, EMPTY], level=2)         # no read at all
    assert text.count(b"\n") == sum(lengths) and text.endswith(b"e5\t5\tN\t0\t*\t*\t0\t*\t*\n")
    assert check(ctx, names, lengths, seqs, [EMPTY, EMPTY], level=1) == b""


def test_a_group_boundary(ctx):
    """More tiles than a group of one sample holds (2048), nearly all of them empty, two reads far apart."""
    length = 2049 * T + 3
    ref = ref_of(length, 10)
    p = 2047 * T + 60
    a = records(R(0, 70, "5M", ref[70:75]), R(0, p, "10M", ref[p:p + 10]))
    text = check(ctx, ["c"], [length], [ref], [a], level=1)
    assert text.count(b"\n") == length


def test_batches_and_rounds(ctx, monkeypatch):
    rnd = random.Random(77)
    names, lengths, seqs, samples = random_cohort(rnd, n_samples=5, n_contigs=3, max_len=5 * T, reads=30)
    kw = dict(level=2, mq=True, bp=True, min_baseq=0)
    whole = check(ctx, names, lengths, seqs, samples, **kw)
    assert ctx.mpileup_stats["batches"] == 1 and ctx.mpileup_stats["rounds"] == 1
    for batch in (1, 300, 4096):
        monkeypatch.setenv("MSNV_MPTEXT_BATCH", str(batch))
        assert ctx.mpileup_text(names, lengths, seqs, samples, all_positions=2, output_mq=True, output_bp=True, min_baseq=0) == whole
        assert ctx.mpileup_stats["batches"] > 1 and ctx.mpileup_stats["text_bytes"] == len(whole) and ctx.mpileup_stats["lines"] == whole.count(b"\n")
    monkeypatch.delenv("MSNV_MPTEXT_BATCH")
    monkeypatch.setenv("MSNV_MPTEXT_ROUND", "2")
    assert ctx.mpileup_text(names, lengths, seqs, samples, all_positions=2, output_mq=True, output_bp=True, min_baseq=0) == whole
    assert ctx.mpileup_stats["rounds"] == 3 and ctx.mpileup_stats["samples"] == 5


# ------------------------------------------------------------------------------------------------ 6. statistics
def test_statistics_with_the_options_on(ctx):
    names, lengths, seqs, samples = random_cohort(random.Random(6), n_samples=3, n_contigs=2)
    text = ctx.mpileup_text(names, lengths, seqs, samples, all_positions=2, output_mq=True, output_bp=True)
    st = ctx.mpileup_stats
    assert st["lines"] == text.count(b"\n") == sum(lengths) + sum(1 for ln in text.split(b"\n")[:-1] if int(ln.split(b"\t")[1]) > lengths[int(ln[1:2])])
    assert st["text_bytes"] == len(text) and st["samples"] == 3
    assert st["elements"] == sum(c[2] for c in strip_columns(text.decode("latin-1"), 2)[1])


# ------------------------------------------------------------------------------------------------ 7. the tool
def test_tool(ctx, tmp_path):
    syn, samples = synth_case(n_species=3, contig_len=700, n_samples=2, mean_cov=3.0, read_len=50, frac_absent=0.5, frac_indel_reads=0.2, seed=43)
    fa = str(tmp_path / "ref.fa")
    syn.write_fasta(fa)
    paths = []
    for i, s in enumerate(samples):
        paths.append(str(tmp_path / ("s%d.bam" % i)))
        core.write_bam(paths[-1], syn.names, syn.lengths, s)
    lst, out = str(tmp_path / "all_samples"), str(tmp_path / "out.mp")
    open(lst, "w").write("\n".join(paths) + "\n")
    exe = os.path.join(TOOLS, "msnv_mpileup")
    for argv, kw in ((["-aa", "-s", "-O"], dict(all_positions=2, output_mq=True, output_bp=True)), (["-a", "--output-BP"], dict(all_positions=1, output_bp=True)),
                     (["-a", "-a", "-s"], dict(all_positions=2, output_mq=True))):
        r = subprocess.run([exe, "-f", fa, "-B", "-b", lst] + argv + ["-o", out], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"", r.stderr
        want = ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, **kw)
        assert want.count(b"\n") >= sum(syn.lengths) if kw["all_positions"] == 2 else want
        assert open(out, "rb").read() == want
    st = ctx.mpileup_files(paths, fa, out, all_positions=2, output_mq=True, output_bp=True)      # the Python form of the first call
    assert open(out, "rb").read() == ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, all_positions=2, output_mq=True, output_bp=True)
    assert st["lines"] >= sum(syn.lengths)
