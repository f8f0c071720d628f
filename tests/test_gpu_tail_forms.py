"""The tail of a pass -- msnv_gather_scatter's two halves -- at the smallest shapes where its forms can go wrong, against the oracle.

Scatter half: an allele event lands with a plain two-byte store where its cell has one writer and with an atomic add in tiles that hold a
split sample (finalize.cpp: slots marks those in tile_nslots); its loop takes four events per trip, the last trip with fewer.  Gather half: tiles
with fewer than 32 sites per workgroup deal their threads as pair lanes x site lanes.  Pileup kernel: the events of a thread's eight
positions are counted with a masked byte SAD.

Every cohort is built by hand: error-free reads tile the contig at a fixed depth per sample, and chosen (position, sample) cells carry
chosen numbers of reads of chosen alleles, so the events of a pass and every per-sample count are known."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bamtools as bt
from metasnv_amd import core
from parity import run_product, run_oracle, first_diff

pytestmark = pytest.mark.gpu

READ = 50
TILE = 2048


# Every tile through msnv_gate_sites and msnv_gather_scatter's spill gather and event scatter: no merged groups, no whole-tile items, no
# allele planes, and a tile's pairs in one work item (its events in one sub-list)
ROUTE = {"MSNV_SHALLOW_PIECES": "0", "MSNV_FUSE": "0", "MSNV_ALLELES": "events", "MSNV_LAYOUT": "pieces", "MSNV_ITEM_PIECES": "100000", "MSNV_ITEM_TAPER": "0"}


@pytest.fixture(autouse=True)
def _plain_route(monkeypatch):
    for k, v in ROUTE.items():
        monkeypatch.setenv(k, v)


def _other(ref_base, k=0):
    return [b for b in "ACGT" if b != ref_base][k]


def _reference(L, seed, n_at=()):
    rnd = random.Random(seed)
    ref = [rnd.choice("ACGT") for _ in range(L)]
    for p in n_at:
        ref[p] = "N"
    return "".join(ref)


def _cohort(ref, depths, muts):
    """depths[s]: reads over every position of sample s (a number, or a function of the read's start); muts[(pos, s)] = [(base, n), ...]:
    n of the sample's reads over pos carry `base`, the others the reference's.  Returns (samples, events): events = the (position,
    sample, allele) triples with a mismatching base."""
    L, samples = len(ref), []
    for s, dep in enumerate(depths):
        recs = []
        for start in range(0, L - READ + 1, READ):
            d = dep(start) if callable(dep) else dep
            here = [(p, muts[(p, s)]) for p in range(start, start + READ) if (p, s) in muts]
            assert all(sum(n for _, n in al) <= d for _, al in here), "more mutated reads than the depth"
            for c in range(d):
                q = list(ref[start:start + READ])
                for p, al in here:
                    lo = 0
                    for base, n in al:
                        if lo <= c < lo + n:
                            q[p - start] = base
                        lo += n
                recs.append(bt.make_record(0, start, "%dM" % READ, "".join(q), name="s%dr%dc%d" % (s, start, c)))
        samples.append(bt.records(*recs))
    return samples, sum(1 for (p, s), al in muts.items() for base, n in al if n and base != ref[p])


def _run(ref, samples, **pk):
    p = core.default_params(**dict(dict(min_coverage=1, calling_threshold=2, min_fraction=0.0), **pk))
    pop, ind, info, st, ds, ctx = run_product(["ctg"], [len(ref)], [ref], samples, params=p, return_ds=True)
    sites, smp = ds.results()
    ds.close(); ctx.close()
    orac = run_oracle(["ctg"], [len(ref)], [ref], samples, params=p)
    assert pop == orac[0], "called_SNPs differs, " + first_diff(pop, orac[0])
    assert ind == orac[1], "indiv_called differs, " + first_diff(ind, orac[1])
    assert info["n_pileup_bases"] == orac[3]
    return pop, ind, info, st, sites, smp


def _mixed_tiles():
    """Two tiles.  Sample 0 is 40 deep over tile 0 and 6 deep over tile 1, the others 6 deep everywhere: with MSNV_SPLIT_AT=32 tile 0 holds a
    split sample next to four ordinary slots and tile 1 holds none.  Sites in both tiles: one allele in one sample, one in several, two
    alleles in one sample, the three alleles that differ from the reference in one sample, all four at a reference N (the other reads
    carry N there)."""
    ref = _reference(TILE + 600, 91, n_at=(300, TILE + 300))
    muts = {}
    for t0 in (0, TILE):
        o = lambda p, k=0: _other(ref[t0 + p], k)
        muts[(t0 + 100, 0)] = [(o(100), 5)]
        muts[(t0 + 100, 1)] = [(o(100), 2)]
        muts[(t0 + 101, 0)] = [(o(101), 3), (o(101, 1), 2)]                   # two alleles, one sample
        muts[(t0 + 101, 2)] = [(o(101, 1), 6)]
        muts[(t0 + 102, 0)] = [(o(102), 2), (o(102, 1), 2), (o(102, 2), 2)]   # the three mismatching alleles
        muts[(t0 + 102, 3)] = [(o(102), 1), (o(102, 1), 1), (o(102, 2), 1)]
        muts[(t0 + 300, 0)] = [("A", 1), ("C", 2), ("G", 1), ("T", 2)]        # reference N: all four
        muts[(t0 + 300, 4)] = [("A", 1), ("C", 1), ("G", 2), ("T", 1)]
        muts[(t0 + 455, 4)] = [(o(455), 1)]                                   # below the threshold: an event, no site
        muts[(t0 + 49, 0)] = [(o(49), 6)]                                     # last base of a read, first of the next
        muts[(t0 + 50, 1)] = [(o(50), 6)]
    depths = [lambda start: 40 if start + READ <= TILE else 6, 6, 6, 6, 6]
    return (ref,) + _cohort(ref, depths, muts)


@pytest.fixture(scope="module")
def mixed_tiles():
    return _mixed_tiles()


def test_store_path_and_atomic_path_give_the_same_cells(mixed_tiles, monkeypatch):
    """No split sample anywhere (every event is a plain store), then sample 0 split into several pairs of tile 0 (MSNV_SPLIT_AT=32 on the
    40x run: tile 0 holds both kinds of slot and adds, tile 1 still stores): both equal the oracle and each other, cell by cell."""
    ref, samples, events = mixed_tiles
    pop, ind, info, st, sites, smp = _run(ref, samples)
    assert st["n_events"] == events                                        # one event per (position, sample, allele)
    assert pop.count("\n") + ind.count("\n") >= 8
    monkeypatch.setenv("MSNV_SPLIT_AT", "32")
    monkeypatch.setenv("MSNV_GROUP_DEPTH", "16")
    pop2, ind2, info2, st2, sites2, smp2 = _run(ref, samples)
    assert info2["n_pairs"] >= info["n_pairs"] + 2                         # sample 0's run over tile 0 became >= 3 pairs
    assert st2["n_events"] > events                                        # ... that each write their own events
    assert (pop2, ind2) == (pop, ind)
    assert sites.tobytes() == sites2.tobytes() and smp.tobytes() == smp2.tobytes()
    # the site with the three mismatching alleles, tile 0 and tile 1: 2 + 1 reads of each over the cohort, 2 of each in sample 0, 1 in sample 3
    rows = [i for i in range(len(sites)) if sorted(sites["n"][i].tolist()) == [0, 3, 3, 3]]
    assert len(rows) == 2
    for i, cov0 in zip(rows, (40, 6)):
        assert sorted(smp["n"][i, 0].tolist()) == [0, 2, 2, 2] and sorted(smp["n"][i, 3].tolist()) == [0, 1, 1, 1]
        assert smp["cov"][i].tolist() == [cov0, 6, 6, 6, 6]


def _event_cohort(E):
    """One tile, one work item, exactly E allele events: (position, sample, allele) triples over 8 samples and the three mismatching alleles
    of positions 8 apart.  Every third position holds one read of sample 0 only: an event at a position that is no site."""
    ns = 8
    ref = _reference(1900, 7)
    muts, left = {}, E
    for i, p in enumerate(range(10, len(ref) - 60, 8)):
        for s in (range(ns) if i % 3 else (0,)):
            k = min(left, 3 if i % 2 else 1)
            if k:
                muts[(p, s)] = [(_other(ref[p], j), 2 if i % 3 else 1) for j in range(k)]
            left -= k
    assert left == 0
    return (ref,) + _cohort(ref, [6] * ns, muts)


def _event_count_cases():
    """Runs in a child process with MSNV_SCATTER_BLOCKS=1 (the knob is read once per process): a sub-list is then walked by one workgroup, 256
    events apart, four per trip, so 1 024 events are exactly one full trip of every thread."""
    stride, U = 256, 4
    for E in (0, 1, U * stride - 1, U * stride, U * stride + 1):
        ref, samples, events = _event_cohort(E)
        assert events == E
        pop, ind, info, st, sites, smp = _run(ref, samples)
        assert info["n_work"] == 1, info["n_work"]                          # one work item: every event in sub-list 0, the other 31 empty
        assert st["n_events"] == E, (st["n_events"], E)
        print("events %d: %d sites ok" % (E, len(sites)))


def test_event_sub_lists_around_a_full_trip():
    """Sub-lists of 0, 1, U * stride - 1, U * stride and U * stride + 1 events (U = 4 events per trip, stride = 256 with one workgroup per
    sub-list): no trip, one thread's partial trip, every thread's full trip less one event, exactly full, one event into the second trip."""
    env = dict(os.environ, MSNV_SCATTER_BLOCKS="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p), **ROUTE)
    r = subprocess.run([sys.executable, "-c", "import test_gpu_tail_forms as t; t._event_count_cases()"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(" sites ok") == 5, r.stdout[-3000:]


@pytest.mark.parametrize("gather_split", ["1", "4"])
@pytest.mark.parametrize("n_pairs", [1, 5, 63, 64, 65])
def test_gather_pairs_and_sites_per_workgroup(n_pairs, gather_split, monkeypatch):
    """Four tiles with 0, 1, 31 x split and 32 x split sites: 0, 1, 31 and 32 sites per gather workgroup (32 = GD_MIN_SITES goes through LDS,
    with >= 16 pairs in rows of 16-byte stores), tiles of 1, 5, 63, 64 and 65 pairs (the pair lanes of the few-site form are the power of
    two that holds them), MSNV_GATHER_SPLIT 1 and 4.  With 1 or 5 cells per site the tiles behind the first site start on cells that are no
    multiple of 8."""
    monkeypatch.setenv("MSNV_GATHER_SPLIT", gather_split)
    split = int(gather_split)
    ref = _reference(4 * TILE, 300 + n_pairs)
    muts, n_sites = {}, 0
    for tile, n in ((1, 1), (2, 31 * split), (3, 32 * split)):
        for i in range(n):
            p = tile * TILE + 5 + 15 * i
            muts[(p, 0)] = [(_other(ref[p]), 2)]
            if n_pairs > 1 and i % 2:
                muts[(p, 1 + i % (n_pairs - 1))] = [(_other(ref[p], 1), 1)]
            n_sites += 1
    samples, events = _cohort(ref, [2] * n_pairs, muts)
    pop, ind, info, st, sites, smp = _run(ref, samples)
    assert len(sites) == n_sites and st["n_events"] == events
    assert (smp["cov"] == 2).all()                                         # every pair's coverage byte reached its cell
    assert sorted(np.bincount(sites["pos"] // TILE, minlength=4).tolist()) == sorted([0, 1, 31 * split, 32 * split])


def test_event_count_with_allele_bytes_1_and_254_in_every_byte_lane(monkeypatch):
    """The pileup kernel counts a thread's events as the non-zero bytes of its eight allele words (A | C << 8 | G << 16 | T << 24).  Sample 0
    is 254 deep and stays one pair (MSNV_SPLIT_AT=255); eight consecutive positions -- one thread's -- hold 254 reads of A, C, G, T (bytes
    of 254 in each lane) and, further on, one read of each (bytes of 1); sample 1 adds one read so that the single reads become sites
    too.  n_events and every count are exact."""
    monkeypatch.setenv("MSNV_SPLIT_AT", "255")
    ref = list(_reference(400, 5))
    muts = {}
    for j, b in enumerate("ACGT"):
        for p in (104 + j, 200 + j):
            ref[p] = "CGTA"[j]                                              # (a reference base that differs from the allele)
        muts[(104 + j, 0)] = [(b, 254)]
        muts[(200 + j, 0)] = [(b, 1)]
        muts[(200 + j, 1)] = [(b, 1)]
    ref = "".join(ref)
    samples, events = _cohort(ref, [254, 3], muts)
    pop, ind, info, st, sites, smp = _run(ref, samples)
    assert info["n_pairs"] == 2 and events == 12 and st["n_events"] == 12
    assert len(sites) == 8
    assert smp["n"][:, 0, :].sum(axis=0).tolist() == [255, 255, 255, 255] and smp["n"][:, 1, :].sum(axis=0).tolist() == [1, 1, 1, 1]
    assert sorted(smp["n"][:, 0, :].max(axis=1).tolist()) == [1, 1, 1, 1, 254, 254, 254, 254]
    assert (smp["cov"][:, 0] == 254).all() and (smp["cov"][:, 1] == 3).all()
