"""The mpileup-text generator (tests/textgen.py) and the oracle's snpCall restatement, checked against each other WITHOUT a
device.  Three statements of the answer exist for every text the GPU file (tests/test_gpu_mpileup_text_sizes.py) feeds the
device parser: the generator's by-construction prediction (planted counts + the gates and the calling rule, no parser), the
oracle (oracle/orc_snpcall, a restatement of call_vC.cpp run on the bytes) and the product.  This file pins the first two on
each other, and proves from the bytes alone that every shape reaches the route of csrc/textcall.hip it is named for."""
import os
import re
import subprocess

import pytest

import orc
import textgen as tg
from fuzz_mpileup_text import cases as fuzz_cases

FUZZ_SEEDS, FUZZ_CASES = (1, 2), 150       # tests/test_gpu_mpileup_text_sizes.py runs the same
SNPCALL = os.path.join(orc.ROOT, "oracle", "_ref", "snpCall")
need_snpcall = pytest.mark.skipif(not os.path.exists(SNPCALL), reason="oracle/_ref/snpCall not built (needs real boost: make -C oracle ref BOOST_ROOT=...)")

_cache = {}


def shape(name):
    if name not in _cache:
        _cache.clear()                                                    # (one large text at a time)
        _cache[name] = tg.WELL_FORMED[name]()
    return _cache[name]


@pytest.mark.parametrize("name", list(tg.WELL_FORMED))
def test_oracle_agrees_with_the_prediction(name):
    """Line set, coverage and allele totals and every per-sample cell: the two files are rendered from the planted counts and
    compared with the oracle's byte for byte."""
    t = shape(name)
    n_called = 0
    for kw in tg.SETTINGS:
        rc, pop, ind, err = orc.snpcall_text(t.data, **kw)
        assert rc == 0, err
        want = tg.predict(t, **kw)
        assert pop == want[0]
        assert ind == want[1]
        n_called += pop.count(b"\n") + ind.count(b"\n")
    assert n_called > 0


def test_generator_plants_the_whole_alphabet():
    """Every legal piece occurs in the pools (so the agreement above covers it): the ten counted symbols, * $ N n, '^' in front of
    a sign, a caret, a blank and a byte >= 0x80, +n / -n with 1, 2 and 3 digits, +0, a sign without digits, leading blanks."""
    bl = tg.Builder(7, 4, pool=3000)
    toks = b"\t".join(bl.pool.tok)
    for c in b".,ACGTacgt*$Nn":
        assert bytes([c]) in toks
    for x in (b"^+", b"^-", b"^^", b"^ "):
        assert x in toks
    assert re.search(rb"\^[\x80-\xff]", toks) and re.search(rb"[+-]\d[ACGTNacgtn*]", toks) and re.search(rb"[+-]\d\d[ACGTNacgtn*]", toks)
    assert re.search(rb"[+-]150[ACGTNacgtn*]{150}", toks) and re.search(rb"[+-]0+(?!\d)", toks) and re.search(rb"[+-][^0-9]", toks)
    assert any(t.split(b"\t")[1].startswith(b" ") for t in bl.pool.triple) and any(t.endswith(b"\t") for t in bl.pool.triple)
    # letters behind an indel are counted symbols that must not count: some token holds more A/C/G/T letters than planted counts
    assert any(sum(t.count(x) for x in b"ACGTacgt") > sum(c[1:]) for t, c in zip(bl.pool.tok, bl.pool.cnt))


def test_layout_quirks_are_in_the_shapes():
    t = shape("samples_65")
    last = [ln for ln in t.lines if len(ln.proc) == 65]
    assert any(ln.proc[64] for ln in last) and any(not ln.proc[64] for ln in last)           # a last token that is never processed
    assert any(len(ln.proc) < 65 for ln in t.lines)                                          # samples missing at the end
    assert any(ln.refc in b"acgt" for ln in t.lines) and any(ln.refc == 0 for ln in t.lines)
    assert not shape("long").data.endswith(b"\n")                                            # a last line without newline


@pytest.mark.parametrize("S", tg.SAMPLE_COUNTS)
def test_sample_shapes_sit_on_their_side_of_the_limits(S):
    t = shape("samples_%d" % S)
    assert t.S == S and tg.routes(t)["proc_max"] == S
    first = t.data[:t.data.index(b"\n")]
    assert (first.count(b"\t") + 1 - 3) // 3 == S
    hi = 512 if S > 512 else S // 2
    # lines whose only counted A / C / G / T sit in sample hi + 1 (513 where there are more than 512), and in the last sample
    for s in (hi, S - 1):
        only = [ln for ln in t.lines if len(ln.proc) == S and ln.proc[s] and ln.cnt[s, 1:].max() >= 4
                and (ln.cnt[:, 1:] * ln.proc[:, None]).sum() == ln.cnt[s, 1:].sum()]
        assert len(only) >= 5, s
    # ... and such a call reaches indiv_called: the carrier's cell is the only one that is not 0
    rc, pop, ind, _ = orc.snpcall_text(t.data, **tg.SETTINGS[2])
    cells = [ln.split(b"\t")[5].split(b",")[0].split(b"|")[3:] for ln in ind.splitlines()]
    assert any(c[S - 1] == b"5" and c.count(b"0") == S - 1 for c in cells) and any(c[hi] == b"5" and c.count(b"0") == S - 1 for c in cells)


def test_documented_shape():
    t = shape("documented")
    assert t.S == 160 and t.n_lines > 2000 and 3500 < len(t.data) / t.n_lines < 4700
    r = tg.routes(t)
    assert r["r_long"] == set(range(16)) and {1, 2, 3} <= r["step_straddle_k"] and r["tabs_in_two_steps"] > 1000


def test_long_shapes_reach_the_steps_and_the_lds_edge():
    t = shape("long")
    r = tg.routes(t)
    assert r["r_long"] == set(range(16))                                  # all 16 alignments on lines longer than 1 KB
    assert set(range(1, 20)) <= r["step_straddle_k"] and len(r["step_straddle_k"]) >= 50       # a processed base string across byte 1024 k of the window
    assert r["lds_straddle"] >= 8 and r["lds_behind"] >= 100 and r["tabs_in_two_steps"] >= 100
    sizes = {ln.raw_len for ln in t.lines}
    assert any(1008 <= s < 1024 for s in sizes) and any(1024 < s <= 1040 for s in sizes) and any(2033 <= s <= 2048 for s in sizes)
    assert any(8160 <= s < 8192 for s in sizes) and any(8192 < s <= 8224 for s in sizes) and any(s >= 60000 for s in sizes)
    # a line whose newline is the last byte of the LDS copy, at every alignment
    assert {t.r_of(i) for i, ln in enumerate(t.lines) if ln.raw_len + t.r_of(i) == tg.LDS + 1} == set(range(16))
    # the straddling tokens come at several alignments
    rs = {t.r_of(i) for i, ln in enumerate(t.lines)
          if ln.proc.any() and ((ln.b[ln.proc] + t.r_of(i) < tg.LDS) & (ln.e[ln.proc] + t.r_of(i) > tg.LDS)).any()}
    assert len(rs) >= 6
    c = tg.routes(shape("cut"))
    assert c["lds_straddle"] >= 4 and c["proc_max"] == 202
    assert tg.routes(shape("insertion"))["lds_straddle"] == 20
    m = shape("most_samples")
    assert m.S == 16383 and len(m.lines) == 4 and all(60000 < ln.raw_len < 400000 for ln in m.lines)


@pytest.mark.parametrize("grid", [1024, 3072, 3136])
def test_many_lines_change_size_in_both_directions_per_wavefront(grid):
    """Whatever the grid (12 wavefronts per CU; 3072 on 256 CUs): every wavefront with 16 lines or more sees the number of
    processed samples fall AND rise from one of its lines to the next, so extents left over from its previous line would be read
    if the count of this line's samples were wrong."""
    t = shape("many_lines")
    assert len(t.lines) >= 50000 and t.S == 130
    both, total = tg.both_directions(t, grid, min_lines=15)
    assert total == grid and both == total
    assert {0, 1, 3, 130} <= {int(ln.proc.sum()) for ln in t.lines}
    # lines that end inside a base string: its opening tab is there (tab 3 k + 1), the closing one is the previous line's
    assert sum(1 for ln in t.lines if ln.proc.any() and t.data[ln.off:ln.off + ln.raw_len].count(b"\t") % 3 == 1) > 500


@pytest.mark.parametrize("case", tg.NUL_CASES)
def test_nul_cases_cut_where_they_say(case):
    t = shape("nul_" + case)
    nul = t.data.index(b"\0")
    assert t.data.count(b"\0") == 1
    i = max(k for k, ln in enumerate(t.lines) if ln.off <= nul)
    ln, at = t.lines[i], nul - t.lines[i].off
    assert ln.stripped == max(0, at - 1)
    if case in ("behind_tab_1", "behind_tab_2"):
        assert at - int(ln.e[2]) == int(case[-1]) and ln.proc[1] and not ln.proc[2]           # the tab is there, nothing behind it is
    elif case == "behind_tab_3":
        assert ln.proc[2] and not ln.proc[3]
    elif case == "in_token":
        assert ln.b[2] < at < ln.e[2] and ln.proc[1] and not ln.proc[2]
    elif case[0] in "bw":
        where, r = case.split("_")
        assert t.r_of(i) == int(r[1:]) and at + (t.r_of(i) if where[0] == "w" else 0) == int(where[1:])
        assert ln.proc.any() and ln.raw_len == 9000 and (ln.proc.all() or at < 8000)       # bytes of the line lie behind the NUL
    else:
        assert not ln.proc.any()


@pytest.mark.parametrize("kind", ["symbol_80", "symbol_ff", "symbol_digit", "symbol_R"])
def test_foreign_symbols_are_domain_errors(kind):
    t = tg.shape_foreign(kind)
    assert t.err_line == 42 and tg.predict(t) is None
    rc, pop, _, _ = orc.snpcall_text(t.data, c=1, t=1, p=0.0)
    assert rc == orc.ERR_DOMAIN
    assert pop == tg.predict(tg.keep_until(t, 42), c=1, t=1, p=0.0)[0]    # it stops at that line, not before


def test_which_error_texts():
    for bad, both in (((40, 7000, 31000), None), ((7000, 31000), None), ((), 12000)):
        t, planted = tg.shape_which_error(bad_lines=bad, extra_line=None if both else 12000, both_line=both)
        first = min(list(bad) + [12000])
        assert t.err_line == first and t.n_lines == 32000 and (not bad or first in planted)
        rc, pop, _, _ = orc.snpcall_text(t.data, c=1, t=1, p=0.0)
        assert rc == orc.ERR_DOMAIN
        want = tg.predict(tg.keep_until(t, first), c=1, t=1, p=0.0)[0]
        assert pop == want and want.count(b"\n") > first // 2
    t = tg.shape_most_samples(16384)
    assert t.S == 16384 and orc.snpcall_text(t.data)[0] == 0                # only the product draws a line at 16383


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzzer_seeds_stay_inside_the_error_bounds(seed):
    """At most a quarter of the fuzzer's cases may end in a domain error (they compare nothing but the code), at least 10 must."""
    n = n_err = big = 0
    for raw, kw, _ in fuzz_cases(FUZZ_CASES, seed):
        rc = orc.snpcall_text(raw, **kw)[0]
        assert rc in (0, orc.ERR_DOMAIN)
        n += 1
        n_err += rc == orc.ERR_DOMAIN
        big += raw.count(b"\n") > 5 and (raw.split(b"\n")[0].count(b"\t") - 2) // 3 > 512
    assert n == FUZZ_CASES and 10 <= n_err <= n // 4, n_err
    assert big >= 3                                                       # texts of more than 512 samples among them


@need_snpcall
@pytest.mark.parametrize("name", [n for n in tg.WELL_FORMED if not n.startswith("nul_")])
def test_reference_binary_on_the_well_formed_shapes(name, tmp_path):
    t = shape(name)
    for kw in tg.SETTINGS[:2]:
        ip = str(tmp_path / "ind")
        r = subprocess.run([SNPCALL, "-i", ip, "-c", str(kw["c"]), "-t", str(kw["t"]), "-p", str(kw["p"])], input=t.data, capture_output=True, timeout=600)
        with open(ip, "rb") as f:
            ind = f.read()
        rc, pop, oind, _ = orc.snpcall_text(t.data, **kw)
        assert r.returncode == 0 and rc == 0
        assert r.stdout == pop and ind == oind
