"""Allele events of the narrow pileup kernel, from the per-pair pass to the event list, at the shapes where the staging can go wrong.

msnv_pileup_tiles_narrow32 stages, per (sample, tile) pair, the allele word of every position that holds a mismatching allele (kernels.hip:
narrow_pass<LATE>) in a buffer of N_EVCAP = 224 records; the workgroup flushes the buffer from N_EVCAP / 2 records on and behind its last
pair (flush_alleles): one thread per record adds the record's alleles to the tile's totals, sets the individual rule's marks and writes
one event per allele.  A wavefront that finds the buffer full writes its events straight into the list.

Every cohort is built by hand -- error-free reads tile the contig at a fixed depth per sample, chosen (position, sample) cells carry chosen
numbers of reads of chosen alleles -- and every case is compared with the oracle: the two call files byte for byte, and the pass's event
count with the (position, sample, allele) triples of the oracle's own pileup text."""
import random

import pytest

import bamtools as bt
import orc
from metasnv_amd import core
from parity import run_product, run_oracle, first_diff

pytestmark = pytest.mark.gpu

READ = 50
TILE = 2048
N_EVCAP = 224                     # kernels.hip: MSNV_N_EVCAP

# Every tile through the ordinary work items of the narrow kernel and the event route: no merged groups, no whole-tile items, no allele
# planes, the per-piece layout, and a tile's pairs in ONE work item, in sample order (its events in one sub-list)
ROUTE = {"MSNV_SHALLOW_PIECES": "0", "MSNV_FUSE": "0", "MSNV_ALLELES": "events", "MSNV_LAYOUT": "pieces", "MSNV_ITEM_PIECES": "100000", "MSNV_ITEM_TAPER": "0"}


@pytest.fixture(autouse=True)
def _event_route(monkeypatch):
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
    the first n of the sample's reads over pos carry `base`, the next ones the next allele, the rest the reference's."""
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
    return samples


def _pileup_alleles(bases):
    """The mismatching A / C / G / T letters of one sample's base string of an mpileup line."""
    out, i = set(), 0
    while i < len(bases):
        c = bases[i]
        if c == "^":
            i += 2
            continue
        if c in "+-":
            j = i + 1
            while bases[j].isdigit():
                j += 1
            i = j + int(bases[i + 1:j])
            continue
        if c in "ACGTacgt":
            out.add(c.upper())
        i += 1
    return out


def _oracle_triples(ref, samples, p):
    """(position, sample, allele) triples with a mismatching base, counted from the oracle's pileup text."""
    mp = dict(min_baseq=p.min_baseq, flag_filter=p.flag_filter, count_orphans=p.count_orphans, max_depth=p.max_depth, min_mapq=p.min_mapq,
              ignore_overlaps=p.ignore_overlaps)
    n = 0
    for line in orc.mpileup_text(["ctg"], [len(ref)], [ref], samples, mp=mp).splitlines():
        f = line.split("\t")
        for s in range((len(f) - 3) // 3):
            n += len(_pileup_alleles(f[4 + 3 * s]))
    return n


def _run(ref, samples, **pk):
    p = core.default_params(**dict(dict(min_coverage=1, calling_threshold=2, min_fraction=0.0), **pk))
    pop, ind, info, st, ds, ctx = run_product(["ctg"], [len(ref)], [ref], samples, params=p, return_ds=True)
    sites, smp = ds.results()
    ds.close(); ctx.close()
    orac = run_oracle(["ctg"], [len(ref)], [ref], samples, params=p)
    assert pop == orac[0], "called_SNPs differs, " + first_diff(pop, orac[0])
    assert ind == orac[1], "indiv_called differs, " + first_diff(ind, orac[1])
    assert info["n_pileup_bases"] == orac[3]
    assert info["allele_planes"] == 0                                      # the event route, as the dataset reports it
    return pop, ind, info, st, sites, smp, _oracle_triples(ref, samples, p)


@pytest.mark.parametrize("min_snvs", [2, 3, 4])
def test_two_three_and_four_alleles_at_one_position_of_one_sample(min_snvs):
    """One record, several alleles: sample 0 holds two, three and -- at a reference N -- all four alleles at one position, with min_snvs - 1,
    min_snvs and min_snvs + 1 reads (both sides of the individual rule's mark inside one allele word); sample 1 holds one read of some of
    them.  Thresholds 2, 3 and 4."""
    t = min_snvs
    ref = _reference(1900, 40 + t, n_at=(900,))
    o = lambda p, k=0: _other(ref[p], k)
    muts = {
        (100, 0): [(o(100), t - 1), (o(100, 1), t)],
        (101, 0): [(o(101), t), (o(101, 1), t + 1)],
        (600, 0): [(o(600), t - 1), (o(600, 1), t), (o(600, 2), t + 1)],
        (900, 0): [("A", t - 1), ("C", t), ("G", t + 1), ("T", t)],
        (1300, 0): [(o(1300), t - 1)],                                     # below the threshold alone ...
        (1300, 1): [(o(1300), 1)],                                         # ... and reached over the cohort
        (1700, 0): [(o(1700, 2), t + 1)],
        (100, 1): [(o(100), 1)],
        (900, 1): [("G", 1), ("T", 1)],
    }
    samples = _cohort(ref, [4 * t + 2, 3], muts)
    pop, ind, info, st, sites, smp, triples = _run(ref, samples, calling_threshold=t)
    assert info["n_work"] == 1 and info["n_pairs"] == 2
    assert triples == 17 and st["n_events"] == triples
    assert pop.count("\n") + ind.count("\n") >= 5
    row = [i for i in range(len(sites)) if sites["pos"][i] % TILE == 900]
    assert len(row) == 1 and smp["n"][row[0], 0].tolist() == [t - 1, t, t + 1, t] and smp["n"][row[0], 1].tolist() == [0, 0, 1, 1]


def test_sample_split_into_several_pairs_of_a_tile(monkeypatch):
    """Sample 0 is 40 deep: with MSNV_SPLIT_AT=32 and MSNV_GROUP_DEPTH=16 its run is dealt round robin, in start order, into 40 / 16 + 1 = 3
    pairs of the tile (finalize.cpp: split_deep_runs).  Two reads of an allele land in two pairs, one each -- below the threshold in every
    pair, reached in sum: the position goes the unc_bits route and is decided from the per-sample records (msnv_decide_sites); six reads
    land two per pair: the ind4 mark from split pairs.  Every pair writes its own events, so the pass's count is the oracle's triples with a
    split sample's triple counted once per pair that holds it (worked out here from the dealing rule)."""
    monkeypatch.setenv("MSNV_SPLIT_AT", "32")
    monkeypatch.setenv("MSNV_GROUP_DEPTH", "16")
    ref = _reference(1900, 77)
    o = lambda p, k=0: _other(ref[p], k)
    deep, G = 40, 40 // 16 + 1
    muts = {
        (105, 0): [(o(105), 2)],                                           # 1 + 1 in two pairs
        (410, 0): [(o(410), 6)],                                           # 2 + 2 + 2
        (411, 0): [(o(411), 1), (o(411, 1), 2)],                           # two alleles, never two reads in a pair
        (1500, 0): [(o(1500), 1)],                                         # one read: an event, no site
        (1777, 0): [(o(1777), 3), (o(1777, 1), 3), (o(1777, 2), 3)],
        (105, 1): [(o(105, 1), 2)],
        (1500, 2): [(o(1500), 1)],
    }
    samples = _cohort(ref, [deep, 5, 5], muts)
    pop, ind, info, st, sites, smp, triples = _run(ref, samples)
    assert info["n_pairs"] == G + 2
    per_pair = 0                                                           # read c of the reads that start at `start` is piece (start / READ) * deep + c of the run
    for (p, s), al in muts.items():
        lo = 0
        for base, n in al:
            ks = [(p // READ) * deep + c for c in range(lo, lo + n)]
            per_pair += len({k % G for k in ks}) if s == 0 else 1
            lo += n
    assert triples == 10 and per_pair == 20 and st["n_events"] == per_pair
    assert {105, 410, 411, 1500, 1777} <= {int(x) for x in sites["pos"]}


def _staging_cohort(total):
    """One tile, one work item, four pairs in sample order.  Pairs 0 and 1 hold `total` positions with an allele between them -- pair 0 as
    many as stay below the flush trigger -- so the buffer holds exactly `total` records behind pair 1; pair 2 adds ten positions, pair 3 three
    positions with two alleles each (a record that expands to two events)."""
    first = min(total // 2, N_EVCAP // 2 - 1)
    ref = _reference(1900, 1000 + total)
    spots = list(range(8, 1890, 16))                                       # 118 positions, in all four wavefronts' quarters of the tile
    assert first < N_EVCAP // 2 and total - first <= len(spots)
    muts = {}
    for i in range(first):
        p = spots[(7 * i) % len(spots)]                                    # (7 and 118 are coprime: all different)
        muts[(p, 0)] = [(_other(ref[p]), 2 if i % 2 else 1)]
    for i in range(total - first):
        p = spots[i]
        muts[(p, 1)] = [(_other(ref[p], 1), 2 if i % 3 else 1)]
    for i in range(10):
        p = spots[11 * i] + 3
        muts[(p, 2)] = [(_other(ref[p]), 2)]
    for i in range(3):
        p = spots[40 * i] + 5
        muts[(p, 3)] = [(_other(ref[p]), 2), (_other(ref[p], 2), 1)]
    return ref, _cohort(ref, [4, 4, 4, 4], muts), total + 10 + 6


@pytest.mark.parametrize("total", [N_EVCAP // 2 - 1, N_EVCAP // 2, N_EVCAP - 1, N_EVCAP, N_EVCAP + 1])
def test_consecutive_pairs_around_the_flush_trigger_and_a_full_buffer(total):
    """Positions with alleles of two consecutive pairs of one work item that sum to N_EVCAP / 2 - 1 (no flush before the next pair),
    N_EVCAP / 2 (the flush trigger), N_EVCAP - 1, N_EVCAP (a full buffer) and N_EVCAP + 1 (one wavefront of the second pair cannot reserve
    and writes straight into the list), with two more pairs behind them."""
    ref, samples, events = _staging_cohort(total)
    pop, ind, info, st, sites, smp, triples = _run(ref, samples)
    assert info["n_work"] == 1 and info["n_pairs"] == 4
    assert triples == events and st["n_events"] == triples
    assert len(sites) > total // 4


def test_one_pair_with_more_positions_than_the_buffer_next_to_clean_tiles():
    """Three tiles; in the middle one sample 0 holds 300 positions with an allele (every tenth with two): more than the staging buffer takes
    in one pass, so some wavefronts stage and the others write straight into the list, in one pass.  The tiles around it hold one site each.
    MSNV_ALLELES=events keeps the dataset on the event route (asserted from the dataset's info in _run)."""
    ref = _reference(3 * TILE, 555)
    muts = {}
    for i in range(300):
        p = TILE + 20 + 6 * i
        al = [(_other(ref[p]), 2)]
        if i % 10 == 0:
            al.append((_other(ref[p], 1), 1))
        muts[(p, 0)] = al
    for p in (700, 2 * TILE + 900):
        muts[(p, 1)] = [(_other(ref[p]), 2)]
        muts[(p, 2)] = [(_other(ref[p]), 1)]
    samples = _cohort(ref, [5, 3, 3], muts)
    pop, ind, info, st, sites, smp, triples = _run(ref, samples)
    assert triples == 300 + 30 + 4 and st["n_events"] == triples
    assert len(sites) == 302
    per_tile = [sum(1 for x in sites["pos"] if int(x) // TILE == t) for t in range(3)]
    assert per_tile == [1, 300, 1]


@pytest.fixture(scope="module")
def two_depth_tiles():
    """Two tiles: tile 0 holds four samples 4 deep (summed depth bound below 256: the totals' bytes of one word), tile 1 holds sample 0 at 250
    deep next to them (256 and more: two 16-bit halves in two words)."""
    ref = _reference(2 * TILE, 4321, n_at=(300, TILE + 300))
    muts = {}
    for t0 in (0, TILE):
        o = lambda p, k=0: _other(ref[t0 + p], k)
        muts[(t0 + 100, 0)] = [(o(100), 3)]
        muts[(t0 + 100, 1)] = [(o(100), 2)]
        muts[(t0 + 101, 0)] = [(o(101), 2), (o(101, 1), 1)]
        muts[(t0 + 101, 2)] = [(o(101, 1), 4)]
        muts[(t0 + 300, 0)] = [("A", 1), ("C", 1), ("G", 1), ("T", 1)]
        muts[(t0 + 300, 3)] = [("A", 1), ("C", 1), ("G", 2)]
        muts[(t0 + 1999, 3)] = [(o(1999, 2), 1)]
    muts[(TILE + 1200, 0)] = [(_other(ref[TILE + 1200]), 200), (_other(ref[TILE + 1200], 1), 40)]      # counts that need the wider fields
    depths = [lambda start: 250 if start >= TILE + READ else 4, 4, 4, 4]
    return ref, _cohort(ref, depths, muts)


@pytest.mark.parametrize("tot_mode", [None, "2"])
def test_tiles_of_every_total_mode(two_depth_tiles, tot_mode, monkeypatch):
    """The flush adds to the tile's allele totals in the tile's mode (kernels.hip: tot_add_one).  The depth bounds of the two tiles select
    modes 0 and 1; mode 2 needs a summed depth bound of 65 536 -- some 260 samples at the byte bins' limit -- so it is selected the way
    test_allele_total_modes does, with MSNV_TOT_MODE=2, which raises the narrowest mode of every tile."""
    monkeypatch.setenv("MSNV_SPLIT_AT", "255")                             # sample 0 stays one pair of tile 1
    if tot_mode:
        monkeypatch.setenv("MSNV_TOT_MODE", tot_mode)
    ref, samples = two_depth_tiles
    pop, ind, info, st, sites, smp, triples = _run(ref, samples)
    assert info["n_pairs"] == 8
    assert triples == 2 * 13 + 2 and st["n_events"] == triples
    row = [i for i in range(len(sites)) if int(sites["pos"][i]) == TILE + 1200]
    assert len(row) == 1 and sorted(smp["n"][row[0], 0].tolist()) == [0, 0, 40, 200] and smp["cov"][row[0]].tolist() == [250, 4, 4, 4]
