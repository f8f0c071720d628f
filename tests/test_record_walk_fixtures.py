"""The hand-placed streams of tests/test_gpu_record_walk.py hold what their cases are named for: every builder of tests/walkstreams.py
asserts its own property (which record starts how many bytes in front of which seam, which sub-segments hold no record start ...) when
it runs -- here, without a device, so that a fixture that drifts fails loudly instead of testing nothing on the GPU.  The host stage
(csrc/pack.cpp needs no device) takes every sound stream and words every broken one as the fixture says."""
import pytest

import bamtools as bt
import walkstreams as ws
from metasnv_amd import core


@pytest.fixture(autouse=True)
def _host_pack(monkeypatch):
    monkeypatch.setenv("MSNV_PACK", "host")


def _host(c):
    """What the host stage (csrc/pack.cpp; no device needed) says to the case's streams: None, or its error's text."""
    ds = core.Dataset(None, c.names, c.lengths, c.seqs, core.default_params(**c.params))
    try:
        for s in c.samples:
            ds.add_sample_records(s)
    except core._lib.MsnvError as e:
        return str(e).split(": ", 1)[1]
    finally:
        ds.close()
    return None


def test_a_sized_record_has_its_size_and_parses():
    for size in (91, 120, 291, 292, 295, 296, 297, 1000, 71000):
        r = ws.sized(size, 0, 5, "30M", "ACGT" * 7 + "AC", "n")
        assert len(r) == size
        (d,) = list(bt.iter_records(r))
        assert d["pos"] == 5 and d["cigar"] == [(30, 0)] and d["name"].startswith("n")
    st = ws.Stream(64)
    st.read(); st.unm(37); st.tiny(); st.read(kind="filt"); st.fill_to(1000); st.fill_to(2000, "unm")
    assert st.off == 2000 and st.starts[1] == len(st.recs[0]) and [d["pos"] for d in bt.iter_records(st.bytes())][:3] == [20, -1, 23]


@pytest.mark.parametrize("sub", [64, 256])
@pytest.mark.parametrize("build", ws.A_CASES, ids=lambda f: f.__name__)
def test_seam_fixtures(build, sub):
    c = build(sub)
    assert c.sub == sub and all(isinstance(s, ws.Stream) or s.size == 0 for s in c.streams)
    assert _host(c) is None


def test_slot_limit_fixtures():
    for c in (ws.b_cap2(False), ws.b_cap2(True), ws.b_unmapped_tail(), ws.b_field_overflow(), ws.b_two_overhangs(False), ws.b_two_overhangs(True), ws.b_long_element()):
        assert _host(c) is None


def test_boundary_fixtures():
    for what in "abc":
        c = ws.c_bounds(what)
        assert len(c.samples) == len(ws.GAPS) and _host(c) is None
    for c in (ws.c_first_pileup_late(), ws.c_tile_order(False), ws.c_tile_order(True), ws.c_order_at_seams()):
        assert _host(c) is None


@pytest.mark.parametrize("sub", [64, 256, None])
def test_error_fixtures(sub):
    """... and the host's sequential walk words each error as the fixture says: the kind, and for a chain that breaks the byte."""
    built = [ws.d_unsorted_first_of_sub(sub, 1), ws.d_unsorted_first_of_sub(sub, 3), ws.d_unsorted_mid_walk(sub), ws.d_qlen_then_contig(sub),
             ws.d_unsorted_and_qlen(sub, True), ws.d_unsorted_and_qlen(sub, False), ws.d_two_streams(sub)] + [ws.d_cut(sub, cut) for cut in (1, 5, 36, "header")]
    for c, s, r, kind in built:
        msg = _host(c)
        assert msg is not None and msg.startswith(ws.KIND_TEXT[kind]), (kind, msg)
        assert (r is None) == (kind == "malformed BAM record")
        if r is None:
            assert msg == "malformed BAM record at byte %d" % c.bad_byte
        # (the streams in front of the one that fails are sound)
        assert _host(ws.case(c.samples[:s])) is None


def test_failed_guess_fixtures():
    for c in [ws.e_odd_names(first) for first in ws.ODD_NAMES] + [ws.e_pass_limit(), ws.e_big_aux(None), ws.e_big_aux(256)]:
        assert _host(c) is None


def test_wavefront_fixtures():
    for c in [ws.f_n_sub(), ws.f_empty_wavefront(), ws.f_many_streams()] + [ws.f_records_per_wavefront(n) for n in (65, 128, 129)]:
        assert _host(c) is None
