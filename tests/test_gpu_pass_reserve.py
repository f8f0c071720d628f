"""The per-pair pass's reservation in the staging buffer of the narrow pileup kernel, at the seams of a reservation per LANE.

narrow_pass<LATE> (kernels.hip) stages one record per position that holds a mismatching allele.  A thread owns eight consecutive positions
(8 tid .. 8 tid + 7; wavefront w the positions 512 w .. 512 w + 511) and reserves the slots of its positions with one returning add to the
buffer's fill count; the buffer takes N_EVCAP = 224 records and is flushed from N_EVCAP / 2 on, between two pairs.  A reservation that ends
above the cap sends its thread's alleles straight into the event list, and the one that straddles the cap leaves zero records below it.

The cases pin behaviour, not mechanism: whichever thread reserves first, the counts below hold -- every cohort is placed so that the seam is
reached in any order (all threads of the overflowing pair hold the same number of positions, so the k-th reservation starts at the same fill
whoever makes it).  Cohorts, routes and the comparison with the oracle are those of tests/test_gpu_event_flush.py: hand-placed, error-free
50-base reads; both call files byte for byte; the pass's n_events against the oracle's (position, sample, allele) triples."""
import os
import tempfile

import pytest

import test_gpu_event_flush as ef
from metasnv_amd import core
from parity import run_product, run_oracle, first_diff

pytestmark = pytest.mark.gpu

TILE, N_EVCAP, N_PPT = ef.TILE, ef.N_EVCAP, 8
LEN = 1900                                    # one tile; threads 0 .. 236 hold eight positions each


@pytest.fixture(autouse=True)
def _event_route(monkeypatch):
    for k, v in ef.ROUTE.items():
        monkeypatch.setenv(k, v)


def _lanes(muts, ref, sample, tids, np_, alleles=lambda i: 1, base=0):
    """Thread `tid` of the tile at `base` holds alleles at its first np_ positions; alleles(i) of position number i: how many (1 .. 3)."""
    i = 0
    for t in tids:
        for j in range(np_):
            p = base + N_PPT * t + j
            k = alleles(i)
            muts[(p, sample)] = [(ef._other(ref[p], x), 2 if x == 0 and i % 2 else 1) for x in range(k)]
            i += 1
    return muts


def _singles(muts, ref, sample, n, off=3, step=2, base=0):
    """n positions of `sample`, one to a thread (8 * step * i + off), over all four quarters of the tile."""
    assert N_PPT * step * (n - 1) + off < LEN
    for i in range(n):
        p = base + N_PPT * step * i + off
        muts[(p, sample)] = [(ef._other(ref[p], 1), 2 if i % 3 else 1)]
    return muts


def _events(muts):
    return sum(len(al) for al in muts.values())


def _check(ref, muts, depths, **pk):
    pop, ind, info, st, sites, smp, triples = ef._run(ref, ef._cohort(ref, depths, muts), **pk)
    assert triples == _events(muts) and st["n_events"] == triples
    return info, st, sites, smp


def test_the_staging_count_reaches_exactly_the_cap():
    """Pair 0: 111 positions (below the flush trigger: no flush before pair 1).  Pair 1: 113 positions -- fourteen threads with eight, one
    with one: the last reservation, whichever it is, ends at exactly 224.  Nothing has to go past the buffer; two more pairs behind it."""
    ref = ef._reference(LEN, 2240)
    muts = _lanes({}, ref, 0, [17 * i + 1 for i in range(13)], 8)
    _lanes(muts, ref, 0, [235], 7)
    _lanes(muts, ref, 1, [16 * i + 2 for i in range(14)], 8)
    _lanes(muts, ref, 1, [230], 1)
    assert sum(1 for k in muts if k[1] == 0) == N_EVCAP // 2 - 1 and len(muts) == N_EVCAP
    _singles(muts, ref, 2, 10, step=20)
    _lanes(muts, ref, 3, [40, 120, 200], 1, alleles=lambda i: 2)
    info, st, sites, smp = _check(ref, muts, [4, 4, 4, 4])
    assert info["n_work"] == 1 and info["n_pairs"] == 4 and st["n_events"] == N_EVCAP + 10 + 6


@pytest.mark.parametrize("pre,np_,hole", [(111, 8, 1), (109, 8, 3), (105, 8, 7), (109, 4, 3), (111, 2, 1)])
def test_a_reservation_that_straddles_the_cap(pre, np_, hole):
    """Pair 0 leaves `pre` records (no flush).  Every thread of pair 1 that holds anything holds np_ consecutive positions from a multiple of
    8 on, so reservation number (224 - hole - pre) / np_ + 1 starts at 224 - hole in any order: it straddles the cap, `hole` slots stay
    below it, and three more threads reserve above the cap.  Pair 2 stages again behind the flush that saw the hole."""
    fit = (N_EVCAP - hole - pre) // np_
    assert pre < N_EVCAP // 2 and pre + fit * np_ == N_EVCAP - hole and 0 < hole < np_
    ref = ef._reference(LEN, 100 * pre + 10 * np_ + hole)
    muts = _singles({}, ref, 0, pre)
    n = fit + 4
    _lanes(muts, ref, 1, [(236 // n) * i for i in range(n)], np_)
    _singles(muts, ref, 2, 10, off=6, step=11)
    info, st, sites, smp = _check(ref, muts, [4, 4, 4])
    assert info["n_work"] == 1 and info["n_pairs"] == 3 and st["n_events"] == pre + n * np_ + 10


@pytest.mark.parametrize("where", ["one_quarter", "four_quarters"])
def test_far_past_the_cap_inside_one_pass(where):
    """Two tiles; in the second, sample 0 holds 304 positions with an allele (every tenth with two) -- 38 threads of one wavefront's quarter,
    or 38 threads over all four quarters: partly staged, partly straight into the list, in one pass.  Samples 1 and 2 hold a few positions
    in both tiles."""
    ref = ef._reference(TILE + LEN, 3040 + len(where))
    tids = list(range(64, 102)) if where == "one_quarter" else [6 * i for i in range(38)]
    muts = _lanes({}, ref, 0, tids, 8, alleles=lambda i: 2 if i % 10 == 0 else 1, base=TILE)
    assert sum(1 for k in muts) == 304 > N_EVCAP
    for base in (0, TILE):
        _singles(muts, ref, 1, 5, off=2, step=40, base=base)
        _singles(muts, ref, 2, 7, off=5, step=30, base=base)
    info, st, sites, smp = _check(ref, muts, [4, 3, 3])
    assert st["n_events"] == 304 + 31 + 2 * 12
    assert sum(1 for x in sites["pos"] if int(x) >= TILE) >= 152


def test_two_and_three_alleles_on_both_sides_of_the_cap():
    """Sample 0: forty threads with eight positions each, 320 in all; positions with one, two and three alleles alternate, so every thread
    holds all three kinds -- the threads that stage and the threads that write straight into the list alike.  Sample 1 adds a read of some."""
    ref = ef._reference(LEN, 323)
    muts = _lanes({}, ref, 0, [5 * i + 3 for i in range(40)], 8, alleles=lambda i: 1 + i % 3)
    _lanes(muts, ref, 1, [5 * i + 3 for i in range(0, 40, 4)], 3)
    info, st, sites, smp = _check(ref, muts, [6, 3])
    assert st["n_events"] == 107 * 1 + 107 * 2 + 106 * 3 + 30
    p = N_PPT * 3 + 1                                                     # two alleles of sample 0 (2 and 1 reads), two reads of the first in sample 1
    row = [i for i in range(len(sites)) if int(sites["pos"][i]) == p]
    assert len(row) == 1 and sorted(smp["n"][row[0], 0].tolist()) == [0, 0, 1, 2] and sorted(smp["n"][row[0], 1].tolist()) == [0, 0, 0, 2]


def test_split_sample_keeps_its_tag_staged_and_direct(monkeypatch):
    """Sample 0 is 40 deep and dealt into three pairs of the tile (MSNV_SPLIT_AT=32, MSNV_GROUP_DEPTH=16: tests/test_gpu_event_flush.py).  It holds
    two reads of an allele at 360 positions: one read each in two of the three pairs -- below the threshold in every pair, reached in sum, so every
    one of the 360 sites is called only if the record's split bit reaches the unc_bits mark.  Each pair holds ~240 of the positions: more than
    the buffer, so the bit travels both in staged records and with the alleles written straight into the list."""
    monkeypatch.setenv("MSNV_SPLIT_AT", "32")
    monkeypatch.setenv("MSNV_GROUP_DEPTH", "16")
    deep, G = 40, 40 // 16 + 1
    ref = ef._reference(LEN, 360)
    muts = {}
    for t in [5 * i for i in range(45)]:
        for j in range(N_PPT):
            p = N_PPT * t + j
            muts[(p, 0)] = [(ef._other(ref[p]), 2)]
    muts[(1899, 0)] = [(ef._other(ref[1899]), 6)]                          # two reads in each pair: the ind4 mark from split pairs
    _singles(muts, ref, 1, 6, off=7, step=35)
    per_pair, in_pair = 0, [0] * G                                         # read c of the reads that start at `start` is piece (start / READ) * deep + c of the run
    for (p, s), al in muts.items():
        lo = 0
        for base, n in al:
            pairs = {((p // ef.READ) * deep + c) % G for c in range(lo, lo + n)} if s == 0 else {G}
            per_pair += len(pairs)
            for g in pairs:
                if g < G:
                    in_pair[g] += 1
            lo += n
    assert min(in_pair) > N_EVCAP                                          # every pair of the split sample overflows the buffer
    pop, ind, info, st, sites, smp, triples = ef._run(ref, ef._cohort(ref, [deep, 5], muts))
    assert info["n_pairs"] == G + 1
    assert triples == 361 + 6 and st["n_events"] == per_pair == 2 * 360 + 3 + 6
    called = {int(x) for x in sites["pos"]}
    assert all(p in called for (p, s) in muts if s == 0)


@pytest.mark.parametrize("tail", [0, 5])
def test_empty_pair_between_full_ones_and_an_overflowing_last_pair(tail):
    """Pairs 0 and 2 hold 240 positions each (more than the buffer), pair 1 none at all: its pass reserves nothing between the flush behind
    pair 0 and pair 2.  tail = 0: pair 2 is the item's last, and the flush behind the chunk loop sees a fill count above the cap; tail = 5: one
    more pair stages five records behind it."""
    ref = ef._reference(LEN, 2400 + tail)
    muts = _lanes({}, ref, 0, [7 * i for i in range(30)], 8)
    _lanes(muts, ref, 2, [7 * i + 3 for i in range(30)], 8)
    depths = [4, 4, 4]
    if tail:
        _singles(muts, ref, 3, tail, step=40)
        depths.append(4)
    info, st, sites, smp = _check(ref, muts, depths)
    assert info["n_work"] == 1 and info["n_pairs"] == len(depths) and st["n_events"] == 480 + tail


def test_two_passes_over_one_dataset_count_the_same():
    """ds.run() twice: the second pass starts from whatever the first left behind.  A stale record replayed by a flush would double a
    per-sample count; counts, records and both files must be those of the first pass, and the oracle's."""
    ref = ef._reference(LEN, 2222)
    muts = _singles({}, ref, 0, 109)
    _lanes(muts, ref, 1, [13 * i for i in range(18)], 8)                  # 109 + 14 * 8 = 221: a straddling reservation with a hole of three, three threads above the cap
    _lanes(muts, ref, 2, [9 * i + 1 for i in range(26)], 8, alleles=lambda i: 1 + (i % 4 == 0))
    samples = ef._cohort(ref, [4, 4, 4], muts)
    p = core.default_params(min_coverage=1, calling_threshold=2, min_fraction=0.0)
    pop, ind, info, st, ds, ctx = run_product(["ctg"], [len(ref)], [ref], samples, params=p, return_ds=True)
    sites, smp = ds.results()
    st2 = ds.run()
    sites2, smp2 = ds.results()
    with tempfile.TemporaryDirectory() as td:
        pp, ip = os.path.join(td, "called_SNPs"), os.path.join(td, "indiv_called")
        ds.write_calls(pp, ip, None, None)
        pop2, ind2 = open(pp).read(), open(ip).read()
    ds.close(); ctx.close()
    orac = run_oracle(["ctg"], [len(ref)], [ref], samples, params=p)
    assert pop == orac[0], "called_SNPs differs, " + first_diff(pop, orac[0])
    assert ind == orac[1], "indiv_called differs, " + first_diff(ind, orac[1])
    assert pop2 == pop and ind2 == ind
    assert st["n_events"] == _events(muts) == ef._oracle_triples(ref, samples, p) and st2["n_events"] == st["n_events"]
    assert st2["n_sites"] == st["n_sites"] and sites.tobytes() == sites2.tobytes() and smp.tobytes() == smp2.tobytes()
