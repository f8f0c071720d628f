"""The text of `samtools mpileup -f REF [-l BED] -B -b LIST [-q -Q -A -x -d --ff]` formatted on the device (msnv_mpileup_text*,
csrc/mptext.cpp + csrc/mptext_k.hip; tools/msnv_mpileup) against the oracle's restatement (oracle/orc_mpileup.c), BYTE FOR BYTE:
every rule of the text in a hand-placed case, the sizes at which the kernels' forms change (tile of T positions, B read descriptors
through LDS, digit counts, batches and rounds), seeded random cohorts, the round trip through msnv_call_from_mpileup, and the tool.

The one documented divergence (the quality character of a deletion / ref-skip element of the first mate in front
of an overlap) is steered around as tests/fuzz_parity.py does: a random cohort with overlapping proper pairs AND D / N operations runs
with ignore_overlaps=1.  Nothing else is excluded."""
import os
import random
import subprocess

import numpy as np
import pytest

import orc
from bamtools import make_record as R, records
from metasnv_amd import core, _lib
from parity import run_product, run_oracle, synth_case, first_diff

pytestmark = pytest.mark.gpu
T, B = core.mpileup_text_geometry()          # positions per tile, read descriptors per LDS batch (csrc/mptext.h)
TOOLS = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools")

REF = "ACGTTGCAACGGATCCTAGA" * 20            # 400 bases
EMPTY = np.zeros(0, np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def same(ctx, names, lengths, seqs, samples, bed=None, **mp):
    """The product's text, which must be the oracle's."""
    want = orc.mpileup_text(names, lengths, seqs, samples, bed=bed, mp=mp).encode("latin-1")
    got = ctx.mpileup_text(names, lengths, seqs, samples, bed=bed, **mp)
    assert got == want, first_diff(got.decode("latin-1"), want.decode("latin-1"))
    st = ctx.mpileup_stats
    assert st["text_bytes"] == len(got) and st["lines"] == got.count(b"\n") and st["samples"] == len(samples)
    return got


def one(ctx, *recs, ref=REF, length=None, **mp):
    """One contig, one sample holding recs."""
    return same(ctx, ["c"], [length or len(ref)], [ref], [records(*recs)], **mp)


# ------------------------------------------------------------------------------------------------ the rules, one hand-placed case each
def test_head_and_tail_on_one_position(ctx):
    assert one(ctx, R(0, 4, "1M", "T", [30])) == b"c\t5\tT\t1\t^].$\t?\n"
    assert one(ctx, R(0, 4, "1M", "G", [30], mapq=0)) == b"c\t5\tT\t1\t^!G$\t?\n"


def test_mapq_characters(ctx):
    text = one(ctx, *[R(0, 10, "3M", "GGA", [20, 21, 22], mapq=q, name="q%d" % q) for q in (0, 93, 94, 255)])
    assert text.split(b"\n")[0] == b"c\t11\tG\t4\t^!.^~.^~.^~.\t5555"


def test_reverse_strand(ctx):
    text = one(ctx, R(0, 0, "6M", "ACGAAG", flag=16), R(0, 0, "6M", "ACGAAG"))
    assert text.split(b"\n")[3] == b"c\t4\tT\t2\taA\tII"


def test_insertions(ctx):
    seq = REF[100:110]
    recs = [R(0, 100, "1M3I5M", seq[0] + "TTT" + seq[1:6], name="behind_first"),
            R(0, 100, "5M2I1M", seq[:5] + "GG" + seq[5], name="before_last"),
            R(0, 100, "2I5M", "CC" + seq[:5], name="leading"),
            R(0, 100, "2I5M", "CC" + seq[:5], name="leading_rev", flag=16)]
    for n in (1, 9, 10, 100):
        recs.append(R(0, 100, "3M%dI3M" % n, seq[:3] + "ACGTN"[n % 5] * n + seq[3:6], name="ins%d" % n, flag=16 if n == 9 else 0))
    text = one(ctx, *recs)
    assert b"+100" + b"A" * 100 in text and b"+9" + b"n" * 9 in text and b"+3TTT" in text and b"+2GG" in text


def test_deletions_at_a_tile_edge_and_over_the_fasta_end(ctx):
    ref = REF[:T + 40]
    recs = [R(0, T - 3, "3M4D3M", ref[T - 3:T] + ref[T + 4:T + 7], name="suffix_on_last_position_of_tile"),
            R(0, T - 2, "2M3D4M", ref[T - 2:T] + ref[T + 3:T + 7], name="first_star_on_tile_start", flag=16),
            R(0, T - 1, "3M2D2M", ref[T - 1:T + 2] + ref[T + 4:T + 6], name="inside_next_tile"),
            R(0, T + 33, "5M10D3M", ref[T + 33:T + 38] + "ACG", name="over_the_fasta_end"),
            R(0, T + 34, "4M9D3M", ref[T + 34:T + 38] + "ACG", name="over_the_fasta_end_rev", flag=16)]
    text = one(ctx, *recs, ref=ref, length=T + 100)
    assert b"-10" + ref[T + 38:T + 40].encode() + b"N" * 8 in text and b"-9" + ref[T + 38:T + 40].lower().encode() + b"n" * 7 in text
    assert b"\t*" in text.replace(b"\t*\t*", b"")


def test_ref_skip_clips_and_eq_x_operations(ctx):
    recs = [R(0, 10, "5M20N5M", REF[10:15] + REF[35:40], name="skip"),
            R(0, 10, "5M20N5M", REF[10:15] + REF[35:40], name="skip_rev", flag=16),
            R(0, 12, "3S5M2S", "TTT" + REF[12:17] + "GG", name="soft"),
            R(0, 12, "2H5M3H", REF[12:17], name="hard"),
            R(0, 13, "2H3S5M1S4H", "AAA" + REF[13:18] + "C", name="both"),
            R(0, 14, "3=2X3=", REF[14:17] + "NN" + REF[19:22], name="eqx"),
            R(0, 14, "8=", "=" * 8, name="eq_bases")]
    text = one(ctx, *recs)
    assert b">" in text and b"<" in text


def test_iupac_bases_and_reference_letters(ctx):
    ref = "ACGTacgtNNRYacgtnACGT" + REF[:40]
    recs = [R(0, 0, "21M", "ACGTACGTACRYRYNNNMKSW", name="fwd"),
            R(0, 0, "21M", "RCGTACGTACRYRYNNNMKSW", name="rev", flag=16),
            R(1, 3, "8M", "ACGTRYN=", name="no_fasta_record"),
            R(1, 3, "8M", "ACGTRYN=", name="no_fasta_record_rev", flag=16)]
    text = same(ctx, ["c", "absent"], [len(ref), 50], [ref, None], [records(*recs)])
    assert b"absent\t4\tN\t2\t^]A^]a\tII" in text


def test_no_reference_at_all(ctx):
    recs = [R(0, 2, "4M2D2M", "AC=TGA"), R(0, 3, "5M", "ACGTN", flag=16)]
    same(ctx, ["c"], [100], None, [records(*recs)])


def test_a_read_over_the_contig_end_and_one_that_starts_beyond_the_fasta(ctx):
    ref = REF[:100]
    recs = [R(0, 95, "10M", ref[95:100] + "ACGTA", name="over"), R(0, 95, "3M4D3M", "ACGTAC", name="del_over", flag=16),
            R(0, 100, "5M", "ACGTA", name="beyond_fasta_is_filtered")]
    text = one(ctx, *recs, ref=ref, length=100)
    assert text.endswith(b"c\t105\tN\t2\tA$c$\tII\n")


def test_a_read_without_seq(ctx):
    recs = [R(0, 5, "4M1D3M", "*", name="noseq"), R(0, 6, "3M", "ACG", [1, 40, 1], name="plain")]
    assert b"\t0\t*\t*\n" in one(ctx, *recs)                 # -Q 13: every element of the first read is below the cutoff
    text = one(ctx, *recs, min_baseq=0)
    assert b"c\t6\t" + REF[5:6].encode() + b"\t1\t^]N\t!\n" in text


def test_quality_cutoffs_and_the_cap_at_126(ctx):
    q = [12, 13, 92, 93, 94, 200, 0, 255]
    recs = [R(0, 20, "8M", REF[20:28], q), R(0, 20, "8M", REF[20:28], q[::-1], flag=16)]
    text = one(ctx, *recs)
    assert b"c\t21\tA\t1\t^],\t~\n" in text and b"c\t23\tG\t2\t.,\t}~\n" in text and b"c\t24\tT\t2\t.,\t~~\n" in text
    one(ctx, *recs, min_baseq=0)
    one(ctx, *recs, min_baseq=93)
    one(ctx, *recs, min_baseq=94)


def test_empty_samples_filtered_cells_and_gaps(ctx):
    a = records(R(0, 10, "5M", REF[10:15]), R(0, 300, "5M", REF[300:305]))
    b = records(R(0, 12, "5M", REF[12:17], [2] * 5), R(1, 0, "3M", "AAA"))
    text = same(ctx, ["c", "d"], [400, 40], [REF, "ACGT" * 10], [a, EMPTY, b])
    lines = text.split(b"\n")
    assert len(lines) - 1 == 5 + 2 + 5 + 3                  # positions 11-17, 301-305, d:1-3; the gaps print nothing
    assert b"c\t16\tC\t0\t*\t*\t0\t*\t*\t0\t*\t*" in text       # covered by a read whose bases are all below -Q: the line exists
    assert same(ctx, ["c"], [400], [REF], [EMPTY, EMPTY]) == b""
    assert same(ctx, ["c"], [400], [REF], []) == b""


def test_two_contigs_and_a_bed_that_clips_both_ends(ctx):
    a = records(R(0, 5, "50M", REF[5:55]), R(0, 40, "30M", REF[40:70], flag=16), R(1, 0, "20M", REF[100:120]), R(1, 10, "20M", REF[110:130]))
    b = records(R(0, 0, "20M", REF[:20]), R(0, 45, "8M", REF[45:53]), R(0, 60, "8M", REF[60:68]), R(1, 25, "5M", REF[125:130]))
    names, lengths, seqs = ["c", "d"], [400, 300], [REF, REF[100:400]]
    same(ctx, names, lengths, seqs, [a, b])
    text = same(ctx, names, lengths, seqs, [a, b], bed=[(0, 10, 50), (1, 5, 12)])
    assert text.startswith(b"c\t11\t") and b"c\t50\t" in text and b"c\t51\t" not in text and b"d\t6\t" in text and b"d\t13\t" not in text
    text = same(ctx, names, lengths, seqs, [a, b], bed=[(1, 0, 300)])            # a contig absent from the BED prints nothing
    assert text.startswith(b"d\t1\t")
    same(ctx, names, lengths, seqs, [a, b], bed=[(0, 46, 47)])                   # the read at 45-52 of sample b overlaps, the one at 60 does not


def test_read_filters(ctx):
    recs = [R(0, 10, "8M", REF[10:18], name="plain", mapq=30),
            R(0, 10, "8M", REF[10:18], name="orphan", flag=1, mapq=10),
            R(0, 11, "8M", REF[11:19], name="proper", flag=3, mapq=19, mtid=0, mpos=200, tlen=300),
            R(0, 11, "8M", REF[11:19], name="dup", flag=0x400, mapq=20),
            R(0, 12, "8M", REF[12:20], name="secondary", flag=0x100, mapq=60),
            R(0, 12, "8M", REF[12:20], name="qcfail", flag=0x200 | 16, mapq=60),
            R(0, 12, "3S", "ACG", name="no_reference_op"),
            R(0, 13, "8M", REF[13:21], name="unmapped", flag=4)]
    one(ctx, *recs)
    one(ctx, *recs, count_orphans=1)
    one(ctx, *recs, min_mapq=20)
    one(ctx, *recs, flag_filter=0x400)
    one(ctx, *recs, flag_filter=0, count_orphans=1, min_mapq=11)


def test_depth_cap(ctx):
    recs = [R(0, 10, "20M", REF[10:30], name="a%d" % i) for i in range(5)] + [R(0, 11 + i, "20M", REF[11 + i:31 + i], name="b%d" % i) for i in range(5)]
    text = one(ctx, *recs, max_depth=3)
    assert text != one(ctx, *recs)
    one(ctx, *recs, max_depth=1)


def test_overlapping_mates(ctx):
    """The quality edit of overlapping proper pairs (no D / N operation in front of the overlap), and -x."""
    a = R(0, 10, "30M", REF[10:40], [30] * 30, flag=0x63, name="p", mtid=0, mpos=25, tlen=45)
    b = R(0, 25, "30M", REF[25:35] + "T" + REF[36:55], [25] * 30, flag=0x93, name="p", mtid=0, mpos=10, tlen=-45)
    text = one(ctx, a, b)
    assert text != one(ctx, a, b, ignore_overlaps=1)


# ------------------------------------------------------------------------------------------------ sizes at which the kernels' forms change
def test_reads_that_end_around_a_tile_edge_and_one_over_three_tiles(ctx):
    ref = REF[:3 * T + 60]
    recs = [R(0, T - 10, "%dM" % n, ref[T - 10:T - 10 + n], name="last_at_%d" % (T - 10 + n - 1)) for n in (9, 10, 11)]      # last base at T - 2, T - 1, T
    recs += [R(0, T - 5, "%dM" % n, ref[T - 5:T - 5 + n], name="ends_%d" % n, flag=16) for n in (4, 5, 6, 7)]               # end (exclusive) at T - 1, T, T + 1, T + 2
    recs.append(R(0, T - 5, "%dM" % (2 * T + 10), ref[T - 5:3 * T + 5], name="three_tiles"))
    recs.append(R(0, 2 * T - 1, "1M", "A", name="last_position_of_a_tile"))
    recs.append(R(0, 2 * T, "1M", "A", name="first_position_of_a_tile"))
    text = one(ctx, *recs, ref=ref)
    assert text.count(b"\n") == 3 * T + 5 - (T - 10)


@pytest.mark.parametrize("n", [B - 1, B, B + 1, 2 * B, 2 * B + 1])
def test_reads_over_one_position_around_the_lds_batch(ctx, n):
    rnd = random.Random(n)
    recs = sorted(((rnd.randrange(30, 50), i) for i in range(n)))
    recs = [R(0, p, "%dM" % (60 - p), REF[p:60], [rnd.randrange(10, 41) for _ in range(60 - p)], name="r%d" % i, flag=16 * (i % 2), mapq=i % 100) for p, i in recs]
    text = one(ctx, *recs)
    assert text.split(b"\n")[25].split(b"\t")[1] == b"56"


def test_digit_counts_of_cnt(ctx):
    samples = [records(*[R(0, 7, "1M", "A", [40], name="r%d" % i) for i in range(n)]) for n in (9, 10, 99, 100, 999, 1000)]
    text = same(ctx, ["c"], [400], [REF], samples)
    f = text.rstrip(b"\n").split(b"\t")
    assert [f[3 + 3 * i] for i in range(6)] == [b"9", b"10", b"99", b"100", b"999", b"1000"]


def test_digit_counts_of_the_position(ctx):
    rnd = random.Random(5)
    ref = "".join(rnd.choice("ACGT") for _ in range(100001))
    recs = [R(0, 5, "10M", ref[5:15]), R(0, 99995, "6M", ref[99995:100001])]
    text = one(ctx, *recs, ref=ref)
    assert b"c\t9\t" in text and b"c\t10\t" in text and b"c\t99999\t" in text and b"c\t100000\t" in text and text.count(b"\n") == 16


def _cohort(n_samples, seed, **kw):
    p = dict(n_species=2, contig_len=1500, n_samples=n_samples, mean_cov=4.0, read_len=75, snv_density=0.02, error_rate=0.01, frac_lowq=0.1,
             frac_indel_reads=0.1, frac_clip_reads=0.1, frac_flagged=0.03, lowercase_ref=1, seed=seed)
    p.update(kw)
    return synth_case(**p)


@pytest.mark.parametrize("n_samples", [1, 3, 64, 65])
def test_sample_counts(ctx, n_samples):
    syn, samples = _cohort(n_samples, 100 + n_samples, mean_cov=2.0 if n_samples > 3 else 8.0)
    same(ctx, syn.names, syn.lengths, syn.seqs, samples)


def test_batches_and_rounds(ctx, monkeypatch):
    syn, samples = _cohort(5, 77, contig_len=1200, mean_cov=6.0)
    whole = same(ctx, syn.names, syn.lengths, syn.seqs, samples)
    assert ctx.mpileup_stats["batches"] == 1 and ctx.mpileup_stats["rounds"] == 1
    monkeypatch.setenv("MSNV_MPTEXT_BATCH", "1")                                  # every tile is a batch
    assert ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples) == whole
    n_tiles = ctx.mpileup_stats["batches"]
    assert n_tiles >= 2 * (1200 // T)
    monkeypatch.setenv("MSNV_MPTEXT_BATCH", str(len(whole) // 7))                 # seven-odd batches: they end inside the contigs
    assert ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples) == whole
    assert 7 <= ctx.mpileup_stats["batches"] < n_tiles
    monkeypatch.delenv("MSNV_MPTEXT_BATCH")
    monkeypatch.setenv("MSNV_MPTEXT_ROUND", "2")                                  # five samples in rounds of two
    assert ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples) == whole
    assert ctx.mpileup_stats["rounds"] == 3 and ctx.mpileup_stats["samples"] == 5


# ------------------------------------------------------------------------------------------------ seeded random cohorts
def test_random_cohorts(ctx):
    """About 200 cohorts with the generator parameters of tests/fuzz_parity.py, cut to the sizes of this file (contigs of at most 5 000
    bases, 65 samples, reads of 150)."""
    rnd = random.Random(20240607)
    bad = []
    for case in range(200):
        contig_len = rnd.choice([300, 1500, 2047, 2048, 2049, 4096, 5000])
        n_species = rnd.choice([1, 1, 2, 3, 5])
        n_samples = rnd.choice([1, 2, 3, 7, 16, 33, 65])
        mean_cov = rnd.choice([0.5, 2, 5, 10, 30, 80])
        budget = 2.5e5                                                            # aligned bases of a cohort: the oracle formats them on one core
        if contig_len * n_species * n_samples * mean_cov > budget:
            mean_cov = max(0.2, budget / (contig_len * n_species * n_samples))
        kw = dict(n_species=n_species, contig_len=contig_len, n_samples=n_samples, mean_cov=mean_cov, read_len=min(rnd.choice([20, 36, 50, 75, 100, 100, 150]), contig_len),
                  sigma_cov=rnd.choice([0.1, 0.5, 1.0]), frac_absent=rnd.choice([0.0, 0.1, 0.5]), snv_density=rnd.choice([0.0, 0.007, 0.05]),
                  error_rate=rnd.choice([0.0, 0.001, 0.02]), frac_lowq=rnd.choice([0.0, 0.1, 0.5]), frac_indel_reads=rnd.choice([0.0, 0.04, 0.3]),
                  frac_clip_reads=rnd.choice([0.0, 0.03, 0.3]), frac_flagged=rnd.choice([0.0, 0.03]), lowercase_ref=rnd.choice([0, 1]),
                  frac_paired=rnd.choice([0.0, 0.0, 0.5, 1.0]), seed=rnd.randrange(1 << 30), frac_aux=rnd.choice([0.0, 0.3, 1.0]), frac_noseq=rnd.choice([0.0, 0.0, 0.05]))
        mp = dict(min_baseq=rnd.choice([0, 13, 13, 30]), max_depth=rnd.choice([8000, 8000, 8000, 60, 7]), min_mapq=rnd.choice([0, 0, 1, 30]),
                  count_orphans=rnd.choice([0, 1]), flag_filter=rnd.choice([0x704, 0x704, 0x400, 0]), ignore_overlaps=rnd.choice([0, 0, 0, 1]))
        if kw["frac_paired"] > 0 and kw["frac_indel_reads"] > 0:                  # the documented divergence: overlapping proper pairs with D / N operations
            mp["ignore_overlaps"] = 1
        syn, samples = synth_case(**kw)
        bed = None
        if rnd.random() < 0.25:
            keep = [t for t in range(n_species) if rnd.random() < 0.6] or [0]
            bed = [(t, rnd.choice([0, 1, 100]), syn.lengths[t] - rnd.choice([0, 0, 37])) for t in keep]
        want = orc.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, bed=bed, mp=mp).encode("latin-1")
        got = ctx.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, bed=bed, **mp)
        if got != want:
            bad.append((case, kw, mp, bed, first_diff(got.decode("latin-1"), want.decode("latin-1"))))
    assert not bad, "%d of 200 cohorts differ; the first: %r" % (len(bad), bad[0])


# ------------------------------------------------------------------------------------------------ round trip and tool
def test_round_trip_through_the_text_caller(ctx, tmp_path):
    """product text -> msnv_call_from_mpileup == msnv_call on the same samples == the oracle."""
    syn, samples = synth_case(n_species=2, contig_len=3000, n_samples=6, mean_cov=10.0, snv_density=0.03, frac_indel_reads=0.05, seed=31)
    text = same(ctx, syn.names, syn.lengths, syn.seqs, samples)
    pp, ip = str(tmp_path / "called"), str(tmp_path / "indiv")
    core.call_from_mpileup(ctx, pp, ip, text=text)
    from_text = open(pp).read(), open(ip).read()
    pop, ind, _, _ = run_product(syn.names, syn.lengths, syn.seqs, samples)
    opop, oind, _, _ = run_oracle(syn.names, syn.lengths, syn.seqs, samples)
    assert len(opop) > 0
    assert from_text == (pop, ind)
    assert (pop, ind) == (opop, oind)


def _write_inputs(tmp_path, syn, samples):
    fa = str(tmp_path / "ref.fa")
    syn.write_fasta(fa)
    paths = []
    for i, s in enumerate(samples):
        paths.append(str(tmp_path / ("s%d.bam" % i)))
        core.write_bam(paths[-1], syn.names, syn.lengths, s)
    lst = str(tmp_path / "all_samples")
    open(lst, "w").write("\n".join(paths) + "\n")
    return fa, paths, lst


def test_tool(ctx, tmp_path):
    """`msnv_mpileup -f REF -B -b LIST | msnv_snpcall ...` on BAM files equals the one-process form of the whole pipe (`msnv_snpcall -b`);
    the text is the oracle's; -o and -l work; a missing -B and an unknown samtools option are refused with status 1."""
    syn, samples = synth_case(n_species=2, contig_len=2500, n_samples=4, mean_cov=10.0, snv_density=0.03, seed=41)
    fa, paths, lst = _write_inputs(tmp_path, syn, samples)
    exe, snp = os.path.join(TOOLS, "msnv_mpileup"), os.path.join(TOOLS, "msnv_snpcall")
    r = subprocess.run([exe, "-f", fa, "-B", "-b", lst], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == orc.mpileup_text(syn.names, syn.lengths, syn.seqs, samples).encode("latin-1")
    i1, i2 = str(tmp_path / "indiv1"), str(tmp_path / "indiv2")
    piped = subprocess.run([snp, "-f", fa, "-i", i1, "-c", "4", "-t", "4"], input=r.stdout, capture_output=True)
    whole = subprocess.run([snp, "-f", fa, "-b", lst, "-i", i2, "-c", "4", "-t", "4"], capture_output=True)
    assert piped.returncode == 0 and whole.returncode == 0, (piped.stderr, whole.stderr)
    assert len(whole.stdout) > 0 and piped.stdout == whole.stdout and open(i1).read() == open(i2).read()
    # options: -o FILE, -l BED, -Q, -q, -A, -x, -d, --ff
    bed, out = str(tmp_path / "split.bed"), str(tmp_path / "out.mp")
    open(bed, "w").write("%s\t1\t%d\n" % (syn.names[1], syn.lengths[1]))
    r = subprocess.run([exe, "-f", fa, "-l", bed, "-B", "-b", lst, "-Q", "20", "-q", "1", "-A", "-x", "-d", "5", "--ff", "0x400", "-o", out], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    mp = dict(min_baseq=20, min_mapq=1, count_orphans=1, ignore_overlaps=1, max_depth=5, flag_filter=0x400)
    assert open(out).read() == orc.mpileup_text(syn.names, syn.lengths, syn.seqs, samples, bed=[(1, 1, syn.lengths[1])], mp=mp)
    # the Python form of the same call
    st = ctx.mpileup_files(paths, fa, out)
    assert open(out, "rb").read() == subprocess.run([exe, "-f", fa, "-B", "-b", lst], capture_output=True).stdout and st["samples"] == 4
    for bad in (["-f", fa, "-b", lst], ["-f", fa, "-B", "-b", lst, "-r", "x:1-2"], ["-f", fa, "-B", "-b", lst, "-E"], ["-f", fa, "-B", "-b", lst, "--rf", "2"],
                ["-f", fa, "-B", "-b", lst, paths[0]], []):
        r = subprocess.run([exe] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and r.stderr, bad
