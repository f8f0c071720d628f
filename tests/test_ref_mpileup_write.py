"""Pins row a1 of the survey wherever samtools exists: the text of tools/msnv_mpileup against the text of real
`samtools mpileup -f REF -B -b LIST` on the same BAM files, byte for byte -- and skips where samtools does not exist (this image:
tests/reftools.py searches MSNV_SAMTOOLS, PATH and the usual prefixes).  Single-end reads and NON-overlapping pairs: the one documented
divergence needs overlapping mates, so nothing here is steered around."""
import os
import random
import subprocess

import pytest

import reftools
from bamtools import make_record as R, records
from metasnv_amd import core, _lib
from parity import synth_case

pytestmark = pytest.mark.gpu
SAMTOOLS = reftools.find_samtools()
need_samtools = pytest.mark.skipif(not SAMTOOLS, reason="samtools not found (PATH or MSNV_SAMTOOLS)")
EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools", "msnv_mpileup")


def _write(tmp_path, names, lengths, seqs, samples):
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n" % n)
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    paths = []
    for i, s in enumerate(samples):
        paths.append(str(tmp_path / ("s%d.bam" % i)))
        core.write_bam(paths[-1], names, lengths, s)
    lst = str(tmp_path / "all_samples")
    open(lst, "w").write("\n".join(paths) + "\n")
    return fa, lst


def _both(fa, lst, extra=()):
    ours = subprocess.run([EXE, "-f", fa, "-B", "-b", lst] + list(extra), capture_output=True, timeout=600)
    real = subprocess.run([SAMTOOLS, "mpileup", "-f", fa, "-B", "-b", lst] + list(extra), capture_output=True, timeout=600)
    assert ours.returncode == 0, ours.stderr
    assert real.returncode == 0, real.stderr
    return ours.stdout, real.stdout


@need_samtools
@pytest.mark.parametrize("seed", range(3))
def test_single_end_reads_equal_samtools(tmp_path, seed):
    syn, samples = synth_case(n_species=2, contig_len=4000, n_samples=5, mean_cov=8.0, read_len=100, snv_density=0.02, error_rate=0.01, frac_lowq=0.1,
                              frac_indel_reads=0.1, frac_clip_reads=0.1, frac_flagged=0.03, lowercase_ref=1, frac_aux=0.5, seed=900 + seed)
    seqs = [s.decode() if isinstance(s, bytes) else s for s in syn.seqs]
    fa, lst = _write(tmp_path, syn.names, syn.lengths, seqs, samples)
    ours, real = _both(fa, lst)
    assert len(real) > 0 and ours == real
    ours, real = _both(fa, lst, ["-Q", "0", "-q", "20", "-d", "6"])
    assert ours == real


@need_samtools
def test_non_overlapping_pairs_equal_samtools(tmp_path):
    rnd = random.Random(12)
    ref = "".join(rnd.choice("ACGT") for _ in range(3000))
    samples = []
    for s in range(3):
        recs = []
        for i in range(120):
            a = rnd.randrange(0, 2500)
            b = a + 150 + rnd.randrange(0, 200)                                   # the mate starts behind the first mate's end
            qa, qb = [rnd.randrange(2, 41) for _ in range(100)], [rnd.randrange(2, 41) for _ in range(100)]
            proper = rnd.random() < 0.8
            recs.append((a, R(0, a, "100M", ref[a:a + 100], qa, flag=0x41 | 0x20 | (2 if proper else 0), name="t%d" % i, mtid=0, mpos=b, tlen=b + 100 - a)))
            recs.append((b, R(0, b, "40M2D60M", ref[b:b + 40] + ref[b + 42:b + 102], qb, flag=0x81 | 0x10 | (2 if proper else 0), name="t%d" % i, mtid=0, mpos=a, tlen=-(b + 100 - a))))
        recs.sort(key=lambda x: x[0])
        samples.append(records(*[r for _, r in recs]))
    fa, lst = _write(tmp_path, ["c"], [3000], [ref], samples)
    ours, real = _both(fa, lst)
    assert len(real) > 0 and ours == real
    ours, real = _both(fa, lst, ["-A"])
    assert ours == real
