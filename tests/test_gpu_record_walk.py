"""The front of the device pack (csrc/devpack.hip, csrc/devscan.hip: msnv_scan_sub2 / msnv_scan_sub, msnv_scan_check, msnv_scan_fix / fix2, msnv_sub_bounds,
msnv_scan_write2 / msnv_scan_write, msnv_scan_segments behind them) on HAND-PLACED streams: every record's offset is chosen against the
seams of the walk (multiples of MSNV_SCAN_SUB from a stream's first byte), the slot limits, the boundary search and the order in which
errors are found.  The reference is the host stage's sequential walk (csrc/pack.cpp, MSNV_PACK=host): every column, the per-sample
statistics, the first lines and the calls (packsame._same_dataset), the calls against the oracle too.  Unless a case says otherwise it
runs three ways -- the default route (the quick walk where it may try), MSNV_FRONT=careful and MSNV_SCAN=segments -- and the route taken is
asserted from pack_stats().  The fixtures (tests/walkstreams.py) assert their own placement on the CPU: tests/test_record_walk_fixtures.py."""
import ctypes as C
import re

import numpy as np
import pytest

import walkstreams as ws
from metasnv_amd import core, _lib
from packsame import COLUMNS, _env, _same_dataset
from parity import synth_case

pytestmark = pytest.mark.gpu

ROUTES = {"default": dict(MSNV_FRONT=None, MSNV_SCAN=None), "careful": dict(MSNV_FRONT="careful", MSNV_SCAN=None), "segments": dict(MSNV_FRONT=None, MSNV_SCAN="segments")}


def _route_env(route, sub):
    return dict(ROUTES[route], MSNV_SCAN_SUB=str(sub) if sub else None)


def _run(c, route, oracle=False):
    """One case one way; returns the device pack's statistics."""
    st = {}
    with _env(**_route_env(route, c.sub)):
        _same_dataset(c.names, c.lengths, c.seqs, c.samples, params=core.default_params(**c.params), many=c.many, check_oracle=oracle, stats=st)
    print("%s sub=%s: scan_segments_redone=%d quick_rounds_redone=%d prepass_samples=%d tile_sort_ms=%.3f" %
          (route, c.sub, st["scan_segments_redone"], st["quick_rounds_redone"], st["prepass_samples"], st["tile_sort_ms"]))
    return st


def _three_ways(c, oracle="default", routes=("default", "careful", "segments")):
    return {route: _run(c, route, oracle == route) for route in routes}


def _quick_stood(st):
    """The default route's round went through the quick walk alone: no repair pass, nothing handed to the careful route."""
    assert st["scan_segments_redone"] == 0 and st["quick_rounds_redone"] == 0 and st["prepass_samples"] == 0, st


# ------------------------------------------------------------------------------------------------ A: where a record meets a seam

@pytest.mark.parametrize("sub", [64, 256])
@pytest.mark.parametrize("build", ws.A_CASES, ids=lambda f: f.__name__)
def test_records_at_seams(build, sub):
    """walkstreams.a_*: record starts on and 1 / 3 / 4 / 35 / 36 bytes in front of a seam, at every residue mod 16 behind one, records
    longer than one and than three sub-segments that end at seam - 1 and at seam, streams of a whole number of sub-segments and with a
    last one of 1 / 35 / 36 bytes, a sub-segment whose first record has fewer than two successors, a one-record stream, empty streams."""
    st = _three_ways(build(sub), oracle="default" if sub == 64 else "careful")
    _quick_stood(st["default"])
    assert st["careful"]["scan_segments_redone"] == 0


@pytest.mark.parametrize("sub", [64, 256])
def test_streams_at_seams_read_in_place_at_every_alignment(sub):
    """The streams of test_records_at_seams once more, packed where they lie in ONE device buffer (add_samples_records_resident): stream i
    begins at an offset of residue i mod 16, so guess_entry's aligned 16-byte pieces cut every stream differently -- the seams still count
    from the stream's first byte."""
    streams = [s for build in ws.A_CASES for s in build(sub).samples]
    assert len(streams) >= 16
    hip = C.CDLL("libamdhip64.so")
    offs, o = [], 32
    for i, smp in enumerate(streams):
        o += (i % 16 - o) % 16
        offs.append(o); o += int(smp.size) + 1
    assert {x % 16 for x in offs} == set(range(16))
    cap = o + 256 + 16
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(cap)) == 0
    try:
        assert hip.hipMemset(buf, 0xEE, C.c_size_t(cap)) == 0
        for smp, off in zip(streams, offs):
            a = np.ascontiguousarray(smp, dtype=np.uint8)
            if a.size:
                assert hip.hipMemcpy(C.c_void_p(buf.value + off), C.c_void_p(a.ctypes.data), C.c_size_t(a.size), 1) == 0
        p = core.default_params(min_coverage=1, calling_threshold=1)
        with _env(MSNV_PACK="host"):
            ch = core.Context(0); dh = core.Dataset(ch, ws.NAMES, ws.LENGTHS, ws.SEQS, p)
            for smp in streams:
                dh.add_sample_records(smp)
            ih = dh.finalize()
        with _env(MSNV_PACK="device", **_route_env("default", sub)):
            cd = core.Context(0); dd = core.Dataset(cd, ws.NAMES, ws.LENGTHS, ws.SEQS, p)
            dd.add_samples_records_resident(buf.value, cap, offs, [int(s.size) for s in streams])
            idv = dd.finalize()
        try:
            st = dd.pack_stats()
            assert st["upload_wall_s"] == 0.0
            _quick_stood(st)
            for k in ("n_reads", "n_reads_pileup", "n_pileup_bases", "n_pairs", "n_work"):
                assert ih[k] == idv[k], k
            for col in COLUMNS:
                assert np.array_equal(dh.column(col), dd.column(col)), col
            for s in range(len(streams)):
                assert np.array_equal(dh.sample_stats(s), dd.sample_stats(s)), s
        finally:
            dd.close(); dh.close(); cd.close(); ch.close()
    finally:
        hip.hipFree(buf)


# ------------------------------------------------------------------------------------------------ B: slot limits

def test_exactly_as_many_records_as_slots_and_one_more():
    """MSNV_SCAN_SUB=480, cap2 = 12: a sub-segment of exactly 12 record starts stays on the quick route, one of 13 sends the round to the
    careful route (scan_sub_body: n > cap -> flag 1, scan_fix_body: flag 4), which has slots for every record."""
    st = _three_ways(ws.b_cap2(False))
    _quick_stood(st["default"])
    st = _three_ways(ws.b_cap2(True))
    assert st["default"]["scan_segments_redone"] >= 1 and st["careful"]["scan_segments_redone"] == 0, st


def test_a_run_of_unmapped_records_overflows_the_default_slots():
    """No knob at all: 400 unmapped records of 37 bytes at a sample's end come 167 to a sub-segment of 6144 bytes, which has 130 slots."""
    st = _three_ways(ws.b_unmapped_tail())
    assert st["default"]["scan_segments_redone"] >= 1, st


def test_places_that_do_not_fit_a_slot_field():
    """SubInfo.flags & 8 (SubCnt.odd): SEQ-less reads of 140000M and twice 70000M under -Q 0 at MSNV_SCAN_SUB=8192 -- the round ends on the
    careful route with the host's dataset (the walk itself stands: a round handed back, not a scan redone)."""
    st = _three_ways(ws.b_field_overflow())
    assert st["default"]["quick_rounds_redone"] >= 1 and st["default"]["scan_segments_redone"] == 0, st


def test_two_contigs_overhang_in_one_sub_segment():
    """SubInfo.flags & 4 (SubCnt.odd): the quick route hands the round back (quick_rounds_redone) and the careful route builds it; with a
    seam between the two reads each sub-segment has one overhanging contig and the quick round stands."""
    st = _three_ways(ws.b_two_overhangs(False))
    assert st["default"]["quick_rounds_redone"] >= 1, st
    st = _three_ways(ws.b_two_overhangs(True), oracle=None)
    _quick_stood(st["default"])


def test_a_pileup_element_longer_than_the_slot_holds():
    """maxc_big -> NEED_TOKEN | NEED_BIGC: a deletion of 600000 bases under the default token limit sends the sample through the host
    pre-pass.  The oracle is not asked: its mpileup text would spell the deletion out at every sample's line (600 KB a read); the host pack
    is the reference here, calls included."""
    st = _three_ways(ws.b_long_element(), oracle=None)
    assert st["default"]["prepass_samples"] == 1, st


@pytest.fixture(scope="module")
def plain_cohort():
    syn, samples = synth_case(n_species=1, contig_len=6000, n_samples=2, mean_cov=14.0, snv_density=0.02, seed=51)
    assert all(s.size > 2 * 32768 for s in samples)
    return syn, samples


@pytest.mark.parametrize("sub", [8192, 16384, 32768])
def test_large_sub_segments(plain_cohort, sub):
    """MSNV_SCAN_SUB 8192 (the largest the quick route tries), 16384 and 32768 (the careful walk only: the 16-bit offsets inside a
    sub-segment reach their top) on one plain cohort."""
    syn, samples = plain_cohort
    for route in ("default", "careful") if sub == 8192 else ("default", "segments") if sub == 16384 else ("default",):
        st = {}
        with _env(**_route_env(route, sub)):
            _same_dataset(syn.names, syn.lengths, syn.seqs, samples, many=True, check_oracle=(route == "default" and sub == 32768), stats=st)
        if route == "default":
            assert st["quick_rounds_redone"] == 0 and st["prepass_samples"] == 0, st


# ------------------------------------------------------------------------------------------------ C: what crosses a seam

@pytest.mark.parametrize("what", ["a", "b", "c"])
def test_first_pileup_read_of_a_sub_segment(what):
    """msnv_sub_bounds' backward search: the first pileup read of a sub-segment continues the run and group in front (a), opens a tile (b)
    or a contig (c), with 0, 1 and 3 sub-segments in between that hold only unmapped records, only filtered reads, or no record start."""
    st = _three_ways(ws.c_bounds(what), oracle="default" if what == "a" else None)
    _quick_stood(st["default"])


def test_first_pileup_read_behind_the_first_sub_segment_and_order_at_seams():
    st = _three_ways(ws.c_first_pileup_late())
    _quick_stood(st["default"])
    st = _three_ways(ws.c_order_at_seams(), oracle=None)
    _quick_stood(st["default"])


@pytest.mark.parametrize("across", [False, True], ids=["in_one_sub_segment", "across_a_seam"])
def test_tile_order_flag(across):
    """A read whose first aligned base lies in an earlier tile than its predecessor's: inside a walk (SubInfo.flags & 1) and across a seam
    (msnv_sub_bounds: bflag & 4) the round takes the general tile-order sort."""
    st = _three_ways(ws.c_tile_order(across), oracle="default" if across else None)
    for route in st:
        assert st[route]["tile_sort_ms"] > 0, (route, st[route])
    assert st["default"]["quick_rounds_redone"] == 0 and st["default"]["scan_segments_redone"] == 0


# ------------------------------------------------------------------------------------------------ D: errors

D_CASES = {
    "unsorted_first_of_sub_1_back": lambda sub: ws.d_unsorted_first_of_sub(sub, 1),
    "unsorted_first_of_sub_3_back": lambda sub: ws.d_unsorted_first_of_sub(sub, 3),
    "unsorted_mid_walk": ws.d_unsorted_mid_walk,
    "qlen_then_contig": ws.d_qlen_then_contig,
    "unsorted_and_qlen_mid_walk": lambda sub: ws.d_unsorted_and_qlen(sub, True),
    "unsorted_and_qlen_first_of_sub": lambda sub: ws.d_unsorted_and_qlen(sub, False),
    "streams_0_and_2": ws.d_two_streams,
    "cut_1": lambda sub: ws.d_cut(sub, 1),
    "cut_5": lambda sub: ws.d_cut(sub, 5),
    "cut_36": lambda sub: ws.d_cut(sub, 36),
    "cut_in_header": lambda sub: ws.d_cut(sub, "header"),
}


@pytest.fixture(scope="module")
def ctx():
    c = core.Context(0)
    yield c
    c.close()


def _error(ctx, c, where, env):
    with _env(MSNV_PACK=where, **env):
        ds = core.Dataset(ctx, c.names, c.lengths, c.seqs, core.default_params(**c.params))
        try:
            with pytest.raises(_lib.MsnvError) as e:
                if where == "host":
                    for s in c.samples:
                        ds.add_sample_records(s)
                else:
                    ds.add_samples_records(c.samples)
        finally:
            ds.close()
    assert e.value.code == _lib.EFORMAT, (where, env, str(e.value))
    return str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("sub", [64, 256, None])
@pytest.mark.parametrize("name", list(D_CASES))
def test_errors_name_what_the_host_walk_names(ctx, name, sub):
    """The host's sequential walk (pack.cpp: filter_and_edit) stops at the first bad record and looks, inside one record, at the contig id,
    then at the coordinate order, then at CIGAR against SEQ.  Every device route names the same kind at the hand-placed (sample, record),
    wherever the seams fall; a chain that breaks is worded as the host words it, with the byte inside its stream."""
    c, s, r, kind = D_CASES[name](sub)
    host = _error(ctx, c, "host", {})
    assert host.startswith(ws.KIND_TEXT[kind]), host
    for route in ROUTES:
        dev = _error(ctx, c, "device", _route_env(route, sub))
        print(route, sub, "|", dev, "| host:", host)
        if r is None:
            assert dev == host == "malformed BAM record at byte %d" % c.bad_byte, (route, dev, host)
        else:
            m = re.fullmatch(r"(.*) \(sample (\d+) of the batch, record (\d+)\)", dev)
            assert m, (route, dev)
            assert (m.group(1), int(m.group(2)), int(m.group(3))) == (kind, s, r), (route, dev, host)


# ------------------------------------------------------------------------------------------------ E: guesses that fail

@pytest.mark.parametrize("first", list(ws.ODD_NAMES))
def test_read_names_the_guess_turns_down(first):
    """Every read name begins with a space, with 0x7f or with a UTF-8 letter: hdr_plausible refuses every true header, so every sub-segment
    with a record start is walked again from the true entry -- one repair pass each (both walks: msnv_scan_fix2, msnv_scan_fix)."""
    c = ws.e_odd_names(first)
    st = _three_ways(c, oracle="default" if first == "space" else None)
    for route in ("default", "careful"):
        assert st[route]["scan_segments_redone"] >= c.seams_with_starts, (route, st[route], c.seams_with_starts)
    assert st["default"]["quick_rounds_redone"] == 0


def test_more_repair_passes_than_the_walk_allows():
    """More than 4096 sub-segments that need a repair pass each: SubWalk::settle gives up at 4096, the quick route hands the round to the
    careful one, whose walk gives up in the same way, and msnv_scan_segments takes the round."""
    c = ws.e_pass_limit()
    st = _three_ways(c, oracle=None, routes=("default", "segments"))
    assert st["default"]["scan_segments_redone"] >= 4096, st


@pytest.mark.parametrize("sub", [None, 256])
def test_a_record_with_more_aux_bytes_than_the_guess_accepts(sub):
    st = _three_ways(ws.e_big_aux(sub), oracle="default" if sub else None)
    assert st["default"]["scan_segments_redone"] >= 1 and st["default"]["quick_rounds_redone"] == 0, st


# ------------------------------------------------------------------------------------------------ F: wavefront geometry

def test_rounds_of_63_to_257_sub_segments():
    """wave_records: a wavefront takes 64 consecutive sub-segments; rounds of 63, 64, 65, 255, 256 and 257 (a stream each, added one by one)."""
    st = _three_ways(ws.f_n_sub())
    _quick_stood(st["default"])


def test_a_wavefront_of_sub_segments_without_a_record():
    st = _three_ways(ws.f_empty_wavefront())
    _quick_stood(st["default"])


@pytest.mark.parametrize("n_rec", [65, 128, 129])
def test_more_records_than_lanes_in_a_wavefronts_step(n_rec):
    st = _three_ways(ws.f_records_per_wavefront(n_rec), oracle="default" if n_rec == 129 else None)
    _quick_stood(st["default"])


def test_seventy_short_streams_in_one_round():
    """Sub-segments of many streams in one wavefront, empty streams among them: the statistics go to their own sample's accumulators (the
    mixed-stream branch of msnv_scan_write2's accumulator add) and equal the host's, sample by sample."""
    st = _three_ways(ws.f_many_streams())
    _quick_stood(st["default"])
