"""finalize's routes, each against the oracle and against the default route (KERNELS.md knobs).

Coverage index (devfin.hip: devfin_coverage_launch / devfin_coverage, finalize.cpp: coverage_tables).  The routes and what is compared:
  default          dense (sample, tile) table launched ahead, pair tables / rows / work items cut on the device (msnv_cov_*)
  tables_host      MSNV_COV_TABLES=host: the same runs, the pair tables by the host loops  -> cov_iv, cov_pairs, cov_work BYTE-identical
  late             MSNV_COV_LATE=1: the dense table built inside devfin_coverage, waiting   -> BYTE-identical (the same table, the host's pair
                   tables: the device's and the host's are byte-identical, see tables_host)
  thread           MSNV_COV_THREAD=1: the host's share on a helper thread                  -> BYTE-identical
  sort             MSNV_COV_INDEX=sort: (interval, tile) entries sorted by rocPRIM, runs of equal keys.  The intervals of a (sample, tile) pair
                   may legitimately lie in another order -> compared per (sample, tile) as SORTED MULTISETS of intervals
  dense (forced)   MSNV_COV_INDEX=dense on the sparse cohort that takes the sort form by itself -> the same multiset comparison
Every route's .cov / .cov.detail text (coverage_run and fused_run) and its calls equal the oracle's.

Knobs that finalize reads once per process (MSNV_FINALIZE_TRACE, MSNV_DEPTH_STREAM, MSNV_SCATTER_BLOCKS) and the routes whose proof is a trace
line run in a child (tests/_route_worker.py), one after another.  Knobs of the per-read stage read per call run in this process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from metasnv_amd import core
from packsame import COLUMNS
from parity import run_oracle, synth_case, first_diff

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_route_worker.py")
KNOBS = ["MSNV_COV_INDEX", "MSNV_COV_LATE", "MSNV_COV_TABLES", "MSNV_COV_THREAD", "MSNV_CHUNK_CAP", "MSNV_LAYOUT", "MSNV_SHALLOW_PIECES",
         "MSNV_DEPTH_STREAM", "MSNV_SCATTER_BLOCKS", "MSNV_COV_NARROW_MAX", "MSNV_PACK", "MSNV_FINALIZE", "MSNV_FUSE", "MSNV_FUSE_PIECES",
         "MSNV_MERGE_ALWAYS", "MSNV_TILE_ORDER", "MSNV_NO_ADOPT", "MSNV_DEEP_RELOCATE", "MSNV_DENSE_RELAYOUT"]

TRACE_SORT = r"cov: sort \+ runs \(sync\)"
TRACE_LATE = r"cov: dense table, runs \(sync\)"
TRACE_EARLY_DEV = r"cov: results of the kernels launched ahead, pair tables written there"
TRACE_EARLY_HOST = r"cov: results of the kernels launched ahead\s+-?[0-9.]+ ms"
TRACE_RETRY = r"chunks: cut again with the exact count"
ALL_COV = (TRACE_SORT, TRACE_LATE, TRACE_EARLY_DEV, TRACE_EARLY_HOST)


def _worker(tmp_path, cases, **env):
    """Runs the worker in a fresh child with the knobs given (every other knob of KNOBS unset); returns (stderr, {case: npz})."""
    e = dict(os.environ)
    for k in KNOBS:
        e.pop(k, None)
    e["MSNV_FINALIZE_TRACE"] = "1"
    e.update(env)
    out = tmp_path / ("w%d" % len(list(tmp_path.iterdir())))
    out.mkdir()
    r = subprocess.run([sys.executable, WORKER, str(out)] + list(cases), env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "worker %s %s failed (%d):\n%s\n%s" % (cases, env, r.returncode, r.stdout[-3000:], r.stderr[-5000:])
    return r.stderr, {c: dict(np.load(str(out / (c + ".npz")))) for c in cases}


def _trace(stderr, want, absent=()):
    assert re.search(want, stderr), "route's trace line %r missing:\n%s" % (want, "\n".join(l for l in stderr.splitlines() if "cov:" in l or "chunks" in l))
    for a in absent:
        assert not re.search(a, stderr), "trace line %r of another route:\n%s" % (a, "\n".join(l for l in stderr.splitlines() if "cov:" in l))


def _index_multisets(z, tag=""):
    """{(sample, tile): sorted intervals} from the fetched coverage index (TilePair: sample, lo, hi, row, base lo, base hi; WorkItem: tile,
    pair_lo, pair_hi); every pair belongs to exactly one work item."""
    iv = z[tag + "cov_iv"].view(np.uint32).reshape(-1, 2)
    pairs = z[tag + "cov_pairs"].view(np.uint32).reshape(-1, 8)
    work = z[tag + "cov_work"].view(np.uint32).reshape(-1, 16)
    seen = np.zeros(len(pairs), dtype=np.int32)
    out = {}
    for w in work:
        t, lo, hi = int(w[0]), int(w[1]), int(w[2])
        seen[lo:hi] += 1
        for k in range(lo, hi):
            s, a, b = int(pairs[k, 0]), int(pairs[k, 1]), int(pairs[k, 2])
            base = int(pairs[k, 4]) | int(pairs[k, 5]) << 32
            assert (s, t) not in out, ("two pairs of one (sample, tile)", s, t)
            assert base + b <= len(iv), (s, t, base, b, len(iv))
            out[(s, t)] = sorted(map(tuple, iv[base + a:base + b].tolist()))
    assert (seen == 1).all(), "pairs outside every work item or in two"
    return out


def _same_bytes(a, b, cols, tag=""):
    for c in cols:
        x, y = a[tag + c], b[tag + c]
        assert x.size == y.size, (tag + c, x.size, y.size)
        if not np.array_equal(x, y):
            i = int(np.flatnonzero(x != y)[0])
            raise AssertionError("column %s differs at byte %d of %d" % (tag + c, i, x.size))


COV_COLS = ["cov_iv", "cov_pairs", "cov_work"]
EDGE_TAGS = ["rounds__", "one_round__", "cov15__"]
_cache = {}


def _others(want):
    return tuple(t for t in ALL_COV if t != want)


def _default_cov(tmp_path):
    if "cov" not in _cache:
        err_e, ze = _worker(tmp_path, ["edges"])
        _trace(err_e, TRACE_EARLY_DEV, _others(TRACE_EARLY_DEV))     # (every build of the edges shape: pair tables cut on the device)
        err_w, zw = _worker(tmp_path, ["wide"])
        _trace(err_w, TRACE_EARLY_HOST, _others(TRACE_EARLY_HOST))   # (the wide pair: the device does not cut tables with a pair above 32 767 intervals)
        _cache["cov"] = {"edges": ze["edges"], "wide": zw["wide"]}
    return _cache["cov"]


# route -> (environment, trace line of the edges shape, of the wide shape, comparison with the default route)
COV_ROUTES = {
    "default": ({}, TRACE_EARLY_DEV, TRACE_EARLY_HOST, "bytes"),
    "tables_host": ({"MSNV_COV_TABLES": "host"}, TRACE_EARLY_HOST, TRACE_EARLY_HOST, "bytes"),
    "late": ({"MSNV_COV_LATE": "1"}, TRACE_LATE, TRACE_LATE, "bytes"),
    "thread": ({"MSNV_COV_THREAD": "1"}, TRACE_EARLY_DEV, TRACE_EARLY_HOST, "bytes"),
    "sort": ({"MSNV_COV_INDEX": "sort"}, TRACE_SORT, TRACE_SORT, "multiset"),
}


@pytest.mark.parametrize("route", list(COV_ROUTES))
def test_coverage_index_route(route, tmp_path):
    """Tile seams, contigs of 300 / 2047 / 2048 / 2049 bases, header contigs without reads, an empty sample, a sample below cov_min_mapq,
    cov_max 1 / 10 / 15, a dataset of several rounds and one of a single round (edges); a wide pair and N operations over seams (wide).
    The worker compares every text with the oracle; here the route's trace line and its index against the default route's."""
    env, t_edges, t_wide, how = COV_ROUTES[route]
    base = _default_cov(tmp_path)
    if route == "default":
        got = base
    else:
        err_e, ze = _worker(tmp_path, ["edges"], **env)
        err_w, zw = _worker(tmp_path, ["wide"], **env)
        _trace(err_e, t_edges, _others(t_edges))
        _trace(err_w, t_wide, _others(t_wide))
        got = {"edges": ze["edges"], "wide": zw["wide"]}
    for case, tags in (("edges", EDGE_TAGS), ("wide", ["rounds__"])):
        for tag in tags:
            a, b = got[case], base[case]
            assert np.array_equal(a[tag + "cov_digest"], b[tag + "cov_digest"]), (case, tag, "coverage text")
            assert a[tag + "cov_iv"].size > 0 and a[tag + "cov_pairs"].size > 0
            if how == "bytes":
                _same_bytes(a, b, COV_COLS, tag)
            else:
                ma, mb = _index_multisets(a, tag), _index_multisets(b, tag)
                assert ma.keys() == mb.keys(), (case, tag, sorted(set(ma) ^ set(mb))[:8])
                for k in ma:
                    assert ma[k] == mb[k], (case, tag, "(sample, tile)", k)


def test_sort_form_taken_by_a_sparse_cohort_without_a_knob(tmp_path):
    """640 samples x 8000 tiles > max(8 x intervals, 2^22): the sort form by itself (cov_dense_form).  Every sample's coverage text equals
    the forced dense table's (MSNV_COV_INDEX=dense, launched ahead); the first, the last, the empty and 20 random samples equal the
    oracle (in the worker); the index per (sample, tile) as multisets."""
    err_s, zs = _worker(tmp_path, ["sparse"])
    _trace(err_s, TRACE_SORT, (TRACE_LATE, TRACE_EARLY_DEV, TRACE_EARLY_HOST))
    err_d, zd = _worker(tmp_path, ["sparse"], MSNV_COV_INDEX="dense")
    _trace(err_d, TRACE_EARLY_DEV, (TRACE_SORT, TRACE_LATE))
    a, b = zs["sparse"], zd["sparse"]
    assert len(a["one_round__cov_digest"]) == 640
    assert np.array_equal(a["one_round__cov_digest"], b["one_round__cov_digest"])
    ma, mb = _index_multisets(a, "one_round__"), _index_multisets(b, "one_round__")
    assert ma == mb and len(ma) > 10000


def _chunks(tmp_path, case, cap=None):
    key = (case, cap)
    if key not in _cache:
        env = {"MSNV_SHALLOW_PIECES": "0"}                # (no merged groups: every chunk is a narrow one, cut on the device)
        if cap is not None:
            env["MSNV_CHUNK_CAP"] = str(cap)
        err, z = _worker(tmp_path, [case], **env)
        _cache[key] = (err, z[case])
    return _cache[key]


def _overflow_caps(tmp_path):
    err, z = _chunks(tmp_path, "chunks")
    n = int(z["n_chunks"][0])
    assert n >= 200, n
    return n, [0, 1, n - 1]


def test_chunk_table_overflow_cuts_again_with_the_exact_count(tmp_path):
    """MSNV_CHUNK_CAP below the narrow chunks' number: the device's cut overflows and finalize cuts again with the exact count (finalize.cpp: last_wait).
    The chunk, work item and pair tables are byte-identical to the default route's, calls and coverage equal the oracle (in the worker).
    A cap of exactly the count does not overflow.  The dense layout cuts its chunks on the host: the cap changes nothing there."""
    err0, z0 = _chunks(tmp_path, "chunks")
    assert not re.search(TRACE_RETRY, err0)
    n, caps = _overflow_caps(tmp_path)
    for cap in caps:
        err, z = _chunks(tmp_path, "chunks", cap)
        _trace(err, TRACE_RETRY)
        _same_bytes(z, z0, ["chunks", "work", "pairs"])
    err, z = _chunks(tmp_path, "chunks", n)
    assert not re.search(TRACE_RETRY, err), "a table of exactly the count overflowed"
    _same_bytes(z, z0, ["chunks", "work", "pairs"])
    errd0, zd0 = _chunks(tmp_path, "chunks_dense")
    errd, zd = _chunks(tmp_path, "chunks_dense", 0)
    assert not re.search(TRACE_RETRY, errd)
    assert int(zd0["n_chunks"][0]) >= 200
    _same_bytes(zd, zd0, ["chunks", "work", "pairs"])


def test_chunk_table_overflow_device_bytes(tmp_path):
    """After the retry the first table's bytes no longer count: info()["device_bytes"] is the same for every overflowing cap and no more
    than the default route's (whose table has the bound's room)."""
    _, z0 = _chunks(tmp_path, "chunks")
    n, caps = _overflow_caps(tmp_path)
    got = {cap: int(_chunks(tmp_path, "chunks", cap)[1]["device_bytes"][0]) for cap in caps}
    assert len(set(got.values())) == 1, got
    assert got[0] <= int(z0["device_bytes"][0]), (got, int(z0["device_bytes"][0]))


@pytest.mark.parametrize("env", [{"MSNV_DEPTH_STREAM": "main"}, {"MSNV_SCATTER_BLOCKS": "1"}, {"MSNV_SCATTER_BLOCKS": "64"}],
                         ids=["depth_stream_main", "scatter_blocks_1", "scatter_blocks_64"])
def test_knobs_read_once_per_process(env, tmp_path):
    """The depth stage on the emit kernels' stream; the event scatter with 1 and 64 workgroups a list.  Calls (depth cap 60, so that the
    depth stage has work) and coverage equal the oracle, in the worker."""
    _worker(tmp_path, ["calls"], **env)


# ------------------------------------------------------------------------------------------------ per-read stage knobs (read per call)
def _build_cols(syn, samples, params, one_round=False):
    ctx = core.Context(0)
    ds = core.Dataset(ctx, syn.names, syn.lengths, syn.seqs, params)
    if one_round:
        ds.add_samples_records(samples)
    else:
        for s in samples:
            ds.add_sample_records(s)
    info = ds.finalize()
    st = ds.pack_stats()
    cols = {c: ds.column(c) for c in COLUMNS}
    ds.run()
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        ds.write_calls(td + "/c", td + "/i", None, None)
        texts = open(td + "/c").read(), open(td + "/i").read()
    ds.close(); ctx.close()
    return cols, texts, info, st


SPARSE = dict(n_species=12, contig_len=5000, n_samples=40, mean_cov=12.0, sigma_cov=0.6, snv_density=0.012, frac_absent=0.95, seed=85)

PER_CALL = {
    # knob: (value, synthetic shape, params, one round, columns that must be byte-identical to the default build)
    "MSNV_TILE_ORDER": ("sort", dict(n_species=3, contig_len=20000, n_samples=12, mean_cov=10.0, seed=81), {}, False, COLUMNS),
    "MSNV_DENSE_RELAYOUT": ("host", dict(n_species=2, contig_len=20000, n_samples=10, mean_cov=8.0, read_len=44, seed=82), {}, False, COLUMNS),
    "MSNV_NO_ADOPT": ("1", dict(n_species=2, contig_len=15000, n_samples=8, mean_cov=10.0, seed=83), {}, True, COLUMNS),
    # deep pairs dealt into depth groups; =0 leaves the bases and qualities of such a sample in read order: a layout changed on purpose
    "MSNV_DEEP_RELOCATE": ("0", dict(n_species=1, contig_len=4000, n_samples=3, mean_cov=300.0, sigma_cov=0.3, snv_density=0.02, seed=84), {}, False,
                           ["ref4", "cov_iv", "cov_pairs", "cov_work"]),
    # which pairs take part in whole-tile items (a sparse cohort: fewer than four pairs per covered tile, so the items are on without
    # MSNV_FUSE; pairs of 12-fold coverage hold more than the default 256 pieces): the work items and chunks change on purpose
    "MSNV_FUSE_PIECES=1": ("1", SPARSE, dict(min_coverage=2, calling_threshold=2), False, ["ref4", "cov_iv", "cov_pairs", "cov_work"]),
    "MSNV_FUSE_PIECES=4096": ("4096", SPARSE, dict(min_coverage=2, calling_threshold=2), False, ["ref4", "cov_iv", "cov_pairs", "cov_work"]),
}


def _knob_had_work(knob, i0, i1, s0, s1, c0, c1):
    """That the default build did NOT already take the knob's route, and that the knob's build did: without this a byte comparison with the
    default would hold whatever the knob does."""
    if knob == "MSNV_TILE_ORDER":
        assert s0["tile_sort_ms"] == 0.0 and s1["tile_sort_ms"] > 0.0, (s0["tile_sort_ms"], s1["tile_sort_ms"])
    elif knob == "MSNV_DENSE_RELAYOUT":
        assert s0["dense_samples"] > 0, "no sample in the dense layout"
        assert s1["dense_samples"] == 0, "the dense re-layout still ran on the device"
    elif knob == "MSNV_NO_ADOPT":
        assert s0["columns_adopted"] == 1, "the default build did not adopt its single round's columns"
        assert s1["columns_adopted"] == 0, "the knob's build adopted them"
    elif knob == "MSNV_DEEP_RELOCATE":
        assert s0["deep_runs_split"] > 0, "no deep run was split: the knob had nothing to do"
        assert s1["deep_runs_split"] == 0, "the device form of finalize still dealt the deep runs"
    elif knob.startswith("MSNV_FUSE_PIECES"):
        w0, w1 = i0["n_whole_tile_items"], i1["n_whole_tile_items"]
        assert w0 > 0, "no whole-tile items in the default build: the cohort is not sparse"
        assert (w1 < w0) if knob.endswith("=1") else (w1 > w0), (knob, w0, w1)
        assert not np.array_equal(c0["work"], c1["work"])
    else:
        raise AssertionError("no check for " + knob)


@pytest.mark.parametrize("knob", list(PER_CALL))
def test_per_read_stage_knob(knob, monkeypatch):
    """Each knob against the default build of the same shape: the columns the knob must not change byte for byte (all of test_gpu_devpack's
    COLUMNS for the routes that claim the same build -- tile order by sort, the dense re-layout on host staging, a single round copied
    instead of adopted; the reference and the coverage index where the knob changes the layout on purpose -- the depth groups' bases left
    in read order, the pairs of whole-tile items), and the calls against the oracle.  _knob_had_work proves that the knob changed the route."""
    value, sk, pk, one_round, same = PER_CALL[knob]
    name = knob.split("=")[0]
    for k in KNOBS + [name]:
        monkeypatch.delenv(k, raising=False)
    syn, samples = synth_case(**sk)
    p = core.default_params(**pk)
    c0, t0, i0, s0 = _build_cols(syn, samples, p, one_round)
    monkeypatch.setenv(name, value)
    c1, t1, i1, s1 = _build_cols(syn, samples, p, one_round)
    monkeypatch.delenv(name)
    _knob_had_work(knob, i0, i1, s0, s1, c0, c1)
    for col in same:
        assert c0[col].size == c1[col].size, (knob, col)
        assert np.array_equal(c0[col], c1[col]), (knob, col)
    o = run_oracle(syn.names, syn.lengths, syn.seqs, samples, params=p)
    for t in (t0, t1):
        assert t[0] == o[0], (knob, first_diff(t[0], o[0]))
        assert t[1] == o[1], (knob, first_diff(t[1], o[1]))
    assert i0["n_pileup_bases"] == i1["n_pileup_bases"] == o[3]
