"""The mpileup-text kernel (msnv_parse_pileup_lines, csrc/textcall.hip) at the sizes where its routes change: more than 64
samples (a lane loops over its samples), more than 512 (base-string extents in memory instead of LDS), lines longer than 1 KB
(the tab count carried from step to step, all 16 alignments of a line), longer than the 8192 bytes kept in LDS (tokens read
from memory), many lines per wavefront (LDS and per-wavefront rows reused), NUL and foreign bytes, and which error is named.

The texts come from tests/textgen.py.  The reference of every comparison is the oracle's restatement of call_vC.cpp
(oracle/orc_snpcall) run as a process on the same BYTES; tests/test_textgen.py pins that oracle, without a device, on the
generator's by-construction prediction for the same texts and proves that each text reaches the route it is named for."""
import os
import re
import subprocess

import pytest

import orc
import textgen as tg
from fuzz_mpileup_text import cases as fuzz_cases
from metasnv_amd import core, _lib
from test_textgen import FUZZ_CASES, FUZZ_SEEDS

pytestmark = pytest.mark.gpu


def product(data, tmp_path, chunk=None, **kw):
    """(called_SNPs, indiv_called, stats) of the device path on the bytes `data`; kw: c, t, p like snpCall's options."""
    ctx = core.Context(0)
    pp, ip = str(tmp_path / "called"), str(tmp_path / "indiv")
    for f in (pp, ip):
        if os.path.exists(f):
            os.remove(f)
    p = core.default_params(min_coverage=kw.get("c", 4), calling_threshold=kw.get("t", 4), min_fraction=kw.get("p", 0.01))
    old = os.environ.pop("MSNV_TEXT_CHUNK", None)
    if chunk is not None:
        os.environ["MSNV_TEXT_CHUNK"] = str(chunk)
    try:
        st = core.call_from_mpileup(ctx, pp, ip, text=data, params=p)
    finally:
        ctx.close()
        os.environ.pop("MSNV_TEXT_CHUNK", None)
        if old is not None:
            os.environ["MSNV_TEXT_CHUNK"] = old
    with open(pp, "rb") as f, open(ip, "rb") as g:
        return f.read(), g.read(), st


def first_diff(a, b):
    for k, (x, y) in enumerate(zip(a.split(b"\n"), b.split(b"\n"))):
        if x != y:
            return "output line %d: %r ... != %r ..." % (k + 1, x[:120], y[:120])
    return "lengths %d != %d" % (len(a), len(b))


def same_as_oracle(t, tmp_path, settings=tg.SETTINGS, chunk=None):
    """The product's two files equal the oracle's byte for byte at every setting, and its statistics equal what the generator
    planted.  Returns the last setting's (called_SNPs, indiv_called, stats)."""
    for kw in settings:
        rc, pop, ind, err = orc.snpcall_text(t.data, **kw)
        assert rc == 0, err
        got = product(t.data, tmp_path, chunk=chunk, **kw)
        assert got[0] == pop, first_diff(got[0], pop)
        assert got[1] == ind, first_diff(got[1], ind)
        st = got[2]
        assert st["lines"] == t.n_lines and st["samples"] == t.S
        assert st["called_lines"] == pop.count(b"\n") and st["indiv_lines"] == ind.count(b"\n")
        assert st["base_chars"] == t.base_chars
    return got


def domain_error(data, tmp_path, chunk=None, **kw):
    with pytest.raises(_lib.MsnvError) as e:
        product(data, tmp_path, chunk=chunk, **kw)
    assert e.value.code == _lib.EDOMAIN
    assert not os.path.exists(tmp_path / "called")
    return str(e.value)


# ---------------------------------------------------------------- 1. samples across the lane and LDS-table limits
@pytest.mark.parametrize("S", tg.SAMPLE_COUNTS)
def test_samples_across_the_lane_and_table_limits(S, tmp_path):
    """63 ... 1100 samples; the counted alleles sit in all samples, in s >= 64, in s >= 512 (or the upper half), in sample 513
    alone and in the LAST sample alone in turn; samples without reads, '*', samples missing at the end."""
    t = tg.shape_samples(S)
    pop, ind, st = same_as_oracle(t, tmp_path)
    hi = 512 if S > 512 else S // 2
    cells = [ln.split(b"\t")[5].split(b",")[0].split(b"|")[3:] for ln in ind.splitlines()]
    # the individual call that only sample hi + 1 / only the last sample carries is in indiv_called
    assert any(c[S - 1] == b"5" and c.count(b"0") == S - 1 for c in cells) and any(c[hi] == b"5" and c.count(b"0") == S - 1 for c in cells)


# ---------------------------------------------------------------- 2. the documented shape
def test_documented_shape_through_four_chunk_sizes(tmp_path):
    """160 samples, lines of ~4 KB (the shape KERNELS.md quotes the kernel at): one launch, and MSNV_TEXT_CHUNK values that put
    1, 7 and ~1000 lines into a launch."""
    t = tg.shape_documented()
    pop, ind, st = same_as_oracle(t, tmp_path)
    avg = len(t.data) // t.n_lines
    for chunk in (1, 7 * avg, 1000 * avg):
        got = product(t.data, tmp_path, chunk=chunk, **tg.SETTINGS[-1])
        assert (got[0], got[1]) == (pop, ind), chunk
        assert got[2]["base_chars"] == t.base_chars
    same_as_oracle(t, tmp_path, settings=tg.SETTINGS[:1], chunk=7 * avg)


# ---------------------------------------------------------------- 3. long lines
def test_long_lines_at_all_alignments(tmp_path):
    """Lines of 1 KB +- 16, 2 KB, 8 KB +- 32, lines that end with the LDS copy and lines of 20-100 KB, each at all 16 offsets from a
    16-byte boundary, with tokens across the 1 KB steps and across the LDS edge; the last line has no newline."""
    t = tg.shape_long()
    same_as_oracle(t, tmp_path)
    same_as_oracle(t, tmp_path, settings=tg.SETTINGS[:1], chunk=1)        # one line per launch: every line at r = 0


def test_token_cut_among_200_samples(tmp_path):
    same_as_oracle(tg.shape_cut(), tmp_path)


def test_insertion_announced_in_front_of_the_lds_edge(tmp_path):
    same_as_oracle(tg.shape_insertion_over_the_edge(), tmp_path)


def test_most_samples(tmp_path):
    """16383 samples (lines of ~100 KB; the grid is capped by the per-wavefront rows); 16384 are refused."""
    t = tg.shape_most_samples()
    pop, ind, st = same_as_oracle(t, tmp_path, settings=tg.SETTINGS[:2])
    assert st["samples"] == 16383 and pop.count(b"\n") >= 3
    msg = domain_error(tg.shape_most_samples(16384).data, tmp_path)
    assert "16383" in msg


# ---------------------------------------------------------------- 4. many lines per wavefront
def test_many_lines_per_wavefront_in_one_launch(tmp_path):
    """At least 16 lines per wavefront in ONE launch, their kinds drawn (3 samples' worth of tabs on a line of a 130-sample file,
    full lines, empty lines, lines cut behind field 5 ...): LDS, extents and count rows are reused line after line.  The grid
    is not guessed: the library reports the most lines a wavefront handled (stats[7])."""
    n = 50000                                                             # 16 lines for each of 12 wavefronts on each of 256 CUs, and a few more
    t = tg.shape_many_lines(n)
    pop, ind, st = same_as_oracle(t, tmp_path, settings=tg.SETTINGS[:2])
    if st["lines_per_wave"] < 16:                                         # a larger device: the grid follows from what it reported
        n = n * 17 // max(1, st["lines_per_wave"] - 1)
        t = tg.shape_many_lines(n)
        pop, ind, st = same_as_oracle(t, tmp_path, settings=tg.SETTINGS[:2])
    waves = -(-(t.n_lines - 1) // st["lines_per_wave"])
    print("lines_per_wave = %d (%d lines in one launch: %d wavefronts or a few more)" % (st["lines_per_wave"], t.n_lines - 1, waves))
    assert st["lines_per_wave"] >= 16
    both, total = tg.both_directions(t, waves, min_lines=15)
    assert total > 0 and both == total
    # the same text in launches of ~1000 lines: one or two lines per wavefront
    got = product(t.data, tmp_path, chunk=1000 * (len(t.data) // t.n_lines), **tg.SETTINGS[1])
    assert (got[0], got[1]) == (pop, ind) and got[2]["lines_per_wave"] < 16


# ---------------------------------------------------------------- 5. NUL and foreign bytes
@pytest.mark.parametrize("case", tg.NUL_CASES)
def test_a_nul_ends_the_line(case, tmp_path):
    """strlen: the bytes behind a NUL do not exist and the character in front of it is the one that is dropped -- in the name, in a
    counted base string, 1 / 2 / 3 bytes behind the tab that ends one, as the first byte, and around the 1 KB steps and the LDS
    edge of a 9000-byte line (line bytes at r = 0 and 5, window bytes at r = 5)."""
    t = tg.shape_nul(case)
    same_as_oracle(t, tmp_path)
    same_as_oracle(t, tmp_path, settings=tg.SETTINGS[:1], chunk=1)


def test_high_bytes_behind_a_caret_are_legal(tmp_path):
    same_as_oracle(tg.shape_foreign("caret"), tmp_path)


@pytest.mark.parametrize("kind", ["symbol_80", "symbol_ff", "symbol_digit", "symbol_R"])
def test_foreign_symbols_are_domain_errors(kind, tmp_path):
    t = tg.shape_foreign(kind)
    assert orc.snpcall_text(t.data)[0] == orc.ERR_DOMAIN
    msg = domain_error(t.data, tmp_path)
    byte = {"symbol_80": 0x80, "symbol_ff": 0xff, "symbol_digit": 0x37, "symbol_R": 0x52}[kind]
    assert "mpileup line %d:" % t.err_line in msg and "(0x%02x)" % byte in msg


# ---------------------------------------------------------------- 6. which error is reported
@pytest.mark.parametrize("chunk", [None, 4096])
def test_the_first_bad_line_is_named(chunk, tmp_path):
    """Foreign symbols on lines 40, 7 000 and 31 000 and a sample too many on line 12 000, in one launch (every wavefront reports,
    the smallest line wins) and in launches of 4 KB: the message names the first line and its byte, as the oracle stops there
    (tests/test_textgen.py: its output ends in front of the planted line)."""
    for bad in ((40, 7000, 31000), (7000, 31000)):
        t, planted = tg.shape_which_error(bad_lines=bad)
        assert orc.snpcall_text(t.data, c=1, t=1, p=0.0)[0] == orc.ERR_DOMAIN and t.err_line == bad[0]
        msg = domain_error(t.data, tmp_path, chunk=chunk, c=1, t=1, p=0.0)
        m = re.search(r"mpileup line (\d+): pileup symbol .* \(0x([0-9a-f]{2})\)", msg)
        assert m, msg
        assert (int(m.group(1)), int(m.group(2), 16)) == (bad[0], planted[bad[0]])
    t, _ = tg.shape_which_error(bad_lines=(31000,))
    msg = domain_error(t.data, tmp_path, chunk=chunk)
    assert "mpileup line 12000 holds more samples" in msg
    t, _ = tg.shape_which_error(bad_lines=(), extra_line=None, both_line=12000)
    assert orc.snpcall_text(t.data)[0] == orc.ERR_DOMAIN
    assert "line 12000" in domain_error(t.data, tmp_path, chunk=chunk)


# ---------------------------------------------------------------- 7. the fuzzer's generator
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzzer_cases(seed, tmp_path):
    """tests/fuzz_mpileup_text.py's generator (malformed and well-formed text alike, up to 700 samples, tokens of up to ~1500
    pieces) with fixed seeds: equal outputs, or a domain error on both sides.  A condition, not a measurement: at most a quarter
    of the cases may end in a domain error and at least 10 must (tests/test_textgen.py checks the same with the oracle alone)."""
    n = n_err = 0
    for raw, kw, chunk in fuzz_cases(FUZZ_CASES, seed):
        rc, pop, ind, err = orc.snpcall_text(raw, **kw)
        n += 1
        if rc == orc.ERR_DOMAIN:
            n_err += 1
            domain_error(raw, tmp_path, chunk=chunk, **kw)
        else:
            assert rc == 0, err
            got = product(raw, tmp_path, chunk=chunk, **kw)
            assert got[0] == pop, "case %d: %s" % (n - 1, first_diff(got[0], pop))
            assert got[1] == ind, "case %d: %s" % (n - 1, first_diff(got[1], ind))
    assert n == FUZZ_CASES and 10 <= n_err <= n // 4, n_err


# ---------------------------------------------------------------- 8. the drop-in process
def test_process_drop_in_on_megabytes_of_text(tmp_path):
    """`msnv_snpcall -i INDIV -c 4 -t 4 < mpileup > called_SNPs` with 10 MB on stdin."""
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools", "msnv_snpcall")
    t = tg.shape_documented()
    assert len(t.data) > 8 << 20
    ip = str(tmp_path / "ind")
    r = subprocess.run([exe, "-i", ip, "-c", "4", "-t", "4"], input=t.data, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode("latin-1")
    rc, pop, ind, _ = orc.snpcall_text(t.data, c=4, t=4)
    assert rc == 0 and r.stdout == pop
    with open(ip, "rb") as f:
        assert f.read() == ind
