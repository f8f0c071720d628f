"""qaCompute's -m, -p W and -x FILE on the device (msnv_coverage_extras, csrc/covext_k.hip) against tests/covextmodel.py -- medians,
window sums, region sums and the four files, exactly.

The record sets are those of tests/covmodel.py (lane, tile and contig-end forms, piles of 32 767 / 32 768 intervals, work items of
several pairs, contigs of many tiles); added here: window sizes inside a lane, on lane and tile seams and longer than a tile, on
contigs of every L % W class; a pile on a contig of its own and a sample whose median lies above 65 535 (two refinements of the
histogram window); a sample with
reads in one tile of one contig (the other tiles have no work item: the host's zeros decide the rank; the other contig has no row);
regions on single indices at tile seams, across three tiles, identical, overlapping, in a tile without a work item and on a contig
without a row."""
import os
import subprocess

import numpy as np
import pytest

import covmodel
import covextmodel as xm
import orc
from metasnv_amd import core, _lib

pytestmark = pytest.mark.gpu

TILE = covmodel.TILE
WINDOWS = [1, 31, 32, 33, 2047, 2048, 2049, 5000]
TOOL = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools", "msnv_qacompute")


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def _with_samples(name, extra):
    """The named case of covmodel with further samples behind its own."""
    c = covmodel.cases()[name]
    return covmodel.Case(name + "+", c.names, c.lengths, list(c.samples) + [covmodel.stream(r) for r in extra], cov_max=c.cov_max, seqs=c.seqs)


def _one_tile_sample():
    """Reads in tile 0 of f17 only: 16 tiles of that contig have no work item for the sample, f9 has no row."""
    return [(0, 99, "300M"), (0, 149, "100M"), (0, 1499, "20M")]


_built = {}


def _case(name):
    if name not in _built:
        if name == "f_copies+":
            _built[name] = _with_samples("f_copies", [_one_tile_sample()])
        else:
            _built[name] = covmodel.cases()[name]
        c = _built[name]
        c.dp = [xm.sample_depths(c.lengths, s) for s in c.samples]
    return _built[name]


class _Resident:
    """One finalized dataset per case and module: the runs of a case share it."""
    def __init__(self):
        self.ds = {}

    def get(self, ctx, name):
        if name not in self.ds:
            case = _case(name)
            ds = core.Dataset(ctx, case.names, case.lengths, case.seqs, core.default_params(cov_max=case.cov_max))
            for s in case.samples:
                ds.add_sample_records(s)
            ds.finalize()
            ds.coverage_run()
            self.ds[name] = ds
        return self.ds[name]

    def close(self):
        for ds in self.ds.values():
            ds.close()


@pytest.fixture(scope="module")
def resident(ctx):
    r = _Resident()
    yield r
    r.close()


def _plain_out(case, s):
    return orc.qacompute(case.names, case.lengths, case.samples[s], max_cov=case.cov_max, min_mapq=1)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError("%s differs at %s: %d, the model has %d" % (what, at, got[at], want[at]))


# ------------------------------------------------------------------------------------------------ (a) window sizes
@pytest.mark.parametrize("name", ["d_breaks", "d_ends", "f_copies"])
@pytest.mark.parametrize("W", WINDOWS)
def test_window_sums_and_profile(name, W, ctx, resident, tmp_path):
    case, ds = _case(name), resident.get(ctx, name)
    got = ds.coverage_extras(window=W)
    assert got["launches"] == 1
    want = np.stack([xm.sample_window_sums(case.lengths, dp, W) for dp in case.dp])
    _same(got["window_sums"], want, "%s W=%d window sums" % (name, W))
    assert want.shape[1] == sum(len(xm.window_bounds(int(L), W)) for L in case.lengths)
    for s in range(len(case.samples)):
        out = str(tmp_path / ("s%d" % s))
        ds.write_coverage(s, out, out + ".detail", profile_path=out + ".profile")
        plain = _plain_out(case, s)
        assert open(out + ".profile").read() == xm.profile_text(case.names, case.lengths, case.dp[s], W), (name, W, s)
        assert open(out).read() == plain[0] and open(out + ".detail").read() == plain[1]


# ------------------------------------------------------------------------------------------------ (b) medians
MEDIAN_CASES = (["c_max%d" % m for m in (15, 10, 1)]
                + ["b_%s_32768" % t for t in ("even", "odd", "one_m_in_a_word", "one_m_over_two_words", "one_end")] + ["f_copies+", "d_ends"])


@pytest.mark.parametrize("name", MEDIAN_CASES)
def test_medians(name, ctx, resident, tmp_path):
    case, ds = _case(name), resident.get(ctx, name)
    got = ds.coverage_extras(median=True)
    want = np.stack([xm.medians(case.lengths, dp) for dp in case.dp])
    _same(got["medians"], want, name + " medians")
    if name.startswith("c_max"):
        assert want[15, 0] == 40 and want[3, 0] == 4 and got["launches"] == 1          # depth 40 over 4000 of 6144 positions
    if name.startswith("b_"):                                      # the pile's sample: median 0 beside 32 768 on a few positions
        assert want[1, 0] == 0 and got["launches"] == 1
    if name == "f_copies+":
        assert want[3].tolist() == [0, 0] and got["launches"] == 1
    if name == "d_ends":                                           # contigs of 1 and 2 bases: the last position, below zero, is the median
        assert want[0, :2].tolist() == [-6, -2] and got["launches"] == 1
    for s in range(len(case.samples)):
        out = str(tmp_path / ("s%d" % s))
        ds.write_coverage(s, out, out + ".detail")
        plain = _plain_out(case, s)
        assert open(out).read() == xm.cov_text_with_median(plain[0], len(case.names), want[s]), (name, s)
        assert open(out + ".detail").read() == plain[1]


def test_median_of_the_piles_own_contig(ctx):
    """A pile of 32 768 over more than half of a contig of its own: the median is the pile.  A second sample sits at 1535 and 1536,
    the last depth the first pass counts in a bin of its own and the first one above them; a third holds 70 000 -- a median above
    65 535, which takes both refinements of the histogram window.  (Contigs of 9 and 4101 bases keep the 70 000 records short.)"""
    names, lengths = ["p0", "p1"], [9, 2 * TILE + 5]
    samples = [covmodel.stream([(0, 1, "6M")] * 32768 + [(1, 5, "10M")]),
               covmodel.stream([(1, 100, "2100M")] * 1535 + [(1, 120, "2080M")]),
               covmodel.stream([(0, 1, "6M")] * 70000)]
    dps = [xm.sample_depths(lengths, s) for s in samples]
    ds = core.Dataset(ctx, names, lengths, None, core.default_params())
    try:
        for s in samples:
            ds.add_sample_records(s)
        ds.finalize()
        got = ds.coverage_extras(median=True)
        want = np.stack([xm.medians(lengths, dp) for dp in dps])
        _same(got["medians"], want, "pile medians")
        assert want.tolist() == [[32768, 0], [0, 1536], [70000, 0]] and got["launches"] == 3
        one = ds.coverage_extras(median=True, window=4, regions=[(0, 2, 7)])         # the other consumers run in the first launch only
        _same(one["medians"], want, "pile medians beside the other consumers")
        _same(one["region_sums"], np.stack([xm.region_sums(dp, [(0, 2, 7)]) for dp in dps]), "pile region sums")
        _same(one["window_sums"], np.stack([xm.sample_window_sums(lengths, dp, 4) for dp in dps]), "pile window sums")
    finally:
        ds.close()


# ------------------------------------------------------------------------------------------------ (c) regions
def _regions(name):
    """(contig name, start, end, alias) lines; every line names a header contig."""
    c0 = {"d_breaks": "d0", "f_copies+": "f17"}[name]
    lines = [(c0, i, i, "idx%d" % i) for i in (0, 1, 2047, 2048)]
    lines += [(c0, 2000, 2 * TILE + 100, "three_tiles"), (c0, 2040, 2060, "twin_a"), (c0, 2040, 2060, "twin_b"),
              (c0, TILE + 10, TILE + 500, "overlap_a"), (c0, TILE + 300, TILE + 900, "overlap_b"),
              (c0, 4 * TILE + 10, 4 * TILE + 500, "tile_without_work")]
    if name == "f_copies+":
        lines += [("f9", 100, 5000, "contig_without_row"), ("f9", 0, 9 * TILE - 2, "whole_f9")]
    return lines


@pytest.mark.parametrize("name", ["d_breaks", "f_copies+"])
def test_region_sums_and_specific(name, ctx, resident, tmp_path):
    case, ds = _case(name), resident.get(ctx, name)
    lines = _regions(name)
    triples = [(case.names.index(n), s, e) for n, s, e, _ in lines]
    got = ds.coverage_extras(regions=triples)
    assert got["launches"] == 1
    want = np.stack([xm.region_sums(dp, triples) for dp in case.dp])
    _same(got["region_sums"], want, name + " region sums")
    if name == "d_breaks":
        assert want[0, -1] == 0 and want[0, 4] > 0                       # sample 0 has no read in the contig's last tile
    else:
        assert (want[3, -3:] == 0).all() and (want[0, -3:] > 0).all()    # the one-tile sample: a tile without a work item, a contig without a row
    # the file also names a contig outside the header and one between the header's names in byte order
    file_lines = [("zzz_not_in_header", 3, 9, "outside")] + lines[:5] + [("Absent", 1, 1, "upper_case")] + lines[5:]
    for s in range(len(case.samples)):
        out = str(tmp_path / ("s%d" % s))
        ds.write_coverage(s, out, out + ".detail", specific_path=out + ".specific", regions=file_lines)
        assert open(out + ".specific").read() == xm.specific_text(case.names, case.dp[s], file_lines), (name, s)


def test_regions_outside_their_contig_are_refused(ctx, resident):
    ds = resident.get(ctx, "d_breaks")
    L = 5 * TILE
    for bad in ((0, 5, L), (0, 7, 6), (0, -1, 4)):
        with pytest.raises(_lib.MsnvError) as e:
            ds.coverage_extras(regions=[bad])
        assert e.value.code == _lib.EDOMAIN, bad
    ds.coverage_extras(regions=[(0, L - 1, L - 1)])


# ------------------------------------------------------------------------------------------------ (e) together = alone; nothing = no launch
@pytest.mark.parametrize("name", ["d_breaks", "f_copies+"])
def test_all_three_in_one_run_equal_each_alone(name, ctx, resident):
    case, ds = _case(name), resident.get(ctx, name)
    triples = [(case.names.index(n), s, e) for n, s, e, _ in _regions(name)]
    m = ds.coverage_extras(median=True)
    w = ds.coverage_extras(window=33)
    r = ds.coverage_extras(regions=triples)
    assert not m["window_sums"].size and not m["region_sums"].size and not w["medians"].any()
    both = ds.coverage_extras(median=True, window=33, regions=triples)
    assert both["launches"] == 1
    _same(both["medians"], m["medians"], "medians")
    _same(both["window_sums"], w["window_sums"], "window sums")
    _same(both["region_sums"], r["region_sums"], "region sums")


def test_asking_for_nothing_launches_nothing(ctx, resident):
    got = resident.get(ctx, "d_breaks").coverage_extras()
    assert got["launches"] == 0 and not got["medians"].any() and not got["window_sums"].size and not got["region_sums"].size


# ------------------------------------------------------------------------------------------------ (d) the tool
def test_tool_writes_the_four_files(tmp_path):
    case = _case("e_items")
    s = 4                                                        # reads on e3, e4, e5 only
    bam = str(tmp_path / "s0.bam")
    core.write_bam(bam, case.names, case.lengths, case.samples[s])
    lines = [("e3", 0, 0, "first"), ("nowhere", 1, 2, "outside"), ("e4", 100, 1900, "gene4"), ("e3", 50, 2047, "rest3"), ("e9", 5, 6, "late"), ("e0", 7, 7, "no_reads_here")]
    rfile = str(tmp_path / "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join("%s\t%d\t%d\t%s\n" % ln for ln in lines))
    out = str(tmp_path / "s0.cov")
    r = subprocess.run([TOOL, "-m", "-p", "1000", "-x", rfile, "-c", "10", "-d", "-i", bam, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "Printing details in %s.detail!\n" % out
    dp = case.dp[s]
    assert sorted(dp) == [3, 4, 5]
    plain = _plain_out(case, s)
    assert open(out).read() == xm.cov_text_with_median(plain[0], len(case.names), xm.medians(case.lengths, dp))
    assert open(out + ".detail").read() == plain[1]
    assert open(out + ".profile").read() == xm.profile_text(case.names, case.lengths, dp, 1000)
    assert open(out + ".specific").read() == xm.specific_text(case.names, dp, lines)
    # the argv of metaSNV.py writes what it always wrote, and nothing else
    out2 = str(tmp_path / "plain.cov")
    r = subprocess.run([TOOL, "-c", "10", "-d", "-i", bam, out2], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and open(out2).read() == plain[0] and open(out2 + ".detail").read() == plain[1]
    assert not os.path.exists(out2 + ".profile") and not os.path.exists(out2 + ".specific")


def test_tool_refuses_what_is_not_built(tmp_path):
    bam, out = str(tmp_path / "x.bam"), str(tmp_path / "x.cov")
    r = subprocess.run([TOOL, "-s", "5", "-c", "10", "-d", "-i", bam, out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-s of qaCompute is not supported" in r.stderr
    r = subprocess.run([TOOL, "-p", "0", "-d", "-i", bam, out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage" in r.stderr
    bad = str(tmp_path / "bad.txt")
    with open(bad, "w") as f:
        f.write("e0 1 2 a\ne0 3\n")
    case = _case("e_items")
    core.write_bam(bam, case.names, case.lengths, case.samples[0])
    r = subprocess.run([TOOL, "-x", bad, "-d", "-i", bam, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "multiple of four" in r.stderr
