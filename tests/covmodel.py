"""Test-side model of qaCompute's coverage arithmetic (qaCompute -c N -d -i: the per-contig difference array, its prefix sum,
covSum and the depth histogram), written from the rule in plain int64 numpy, and the hand-placed record sets that
tests/test_gpu_coverage_sizes.py runs msnv_coverage_tiles on.  tests/test_coverage_model.py pins the model against the oracle's
text (oracle/orc_qacompute.c) on every one of those sets; the GPU tests then trust it for the two numbers the text does not
show: hist[0] and the exact covSum.

The rule, for a read that is mapped, has mapq >= min_mapq and is no duplicate (0x400): the cursor starts at pos + 1; a leading
S / H op (the first op only) is skipped without advancing; every other op that is not M advances the cursor by its length; an M op
does +1 at the cursor if the cursor is <= L, advances, then does -1 at the new cursor -- at L - 1 if that is >= L.  depth = prefix
sum over [0, L), covSum = its sum (uint64, so a negative total wraps as the reference's does), hist[min(depth, max_cov)] += 1 for
the positions with depth >= 0 (a position at -1 lands in no bin and still enters the sum).

Rows: the library keeps accumulators for the (sample, contig) combinations that have coverage, and qaCompute prints a contig without
reads and a contig whose reads were all filtered as the same zeros; a contig whose depth is 0 everywhere is a row of zeros here too
(bin 0 included).  Every other row holds all L positions: hist.sum() == L unless the last position went negative."""
import functools

import numpy as np

import bamtools as bt

COV_WORDS = 17                       # covSum, hist[0..15]
TILE = 2048                          # positions per tile of msnv_coverage_tiles
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the model
def marks(lengths, records, min_mapq=1):
    """{tid: (plus, minus, intervals)}: the indices that take +1 / -1, and the M intervals as the coverage index files them --
    (begin, end) with the end clamped to L - 1, (L, L - 1) for "-1 at L - 1 only" (cursor at or beyond L), none where begin >= end."""
    out = {}
    for r in bt.iter_records(records):
        if (r["flag"] & 0x4) or r["tid"] < 0 or r["mapq"] < min_mapq or (r["flag"] & 0x400):
            continue
        L = int(lengths[r["tid"]])
        plus, minus, ivs = out.setdefault(r["tid"], ([], [], []))
        cur = r["pos"] + 1
        ops = r["cigar"]
        for k, (n, op) in enumerate(ops):
            if k == 0 and op in (4, 5):
                continue
            if op != 0:
                cur += n
                continue
            b = cur
            if b <= L:
                plus.append(b)
            cur += n
            e = L - 1 if cur >= L else cur
            minus.append(e)
            if b >= L:
                ivs.append((L, L - 1))
            elif b < e:
                ivs.append((b, e))
    return out


def depths(lengths, mk):
    """{tid: depth[0 .. L)} (int64) of the contigs that have marks."""
    out = {}
    for tid, (plus, minus, _) in mk.items():
        L = int(lengths[tid])
        d = np.zeros(L + 1, dtype=np.int64)
        np.add.at(d, np.asarray(plus, dtype=np.int64), 1)
        np.add.at(d, np.asarray(minus, dtype=np.int64), -1)
        out[tid] = np.cumsum(d[:L])
    return out


def accumulators(lengths, dp, max_cov):
    """[contig][1 + 16] uint64 in the layout of Dataset.coverage_accumulators(): covSum, hist[0 .. 15] (zero above max_cov)."""
    acc = np.zeros((len(lengths), COV_WORDS), dtype=np.uint64)
    for tid, depth in dp.items():
        if not depth.any():
            continue
        acc[tid, 0] = np.uint64(int(depth.sum()) & MASK64)
        h = np.bincount(np.minimum(depth[depth >= 0], max_cov), minlength=16)
        acc[tid, 1:] = h.astype(np.uint64)
    return acc


def pair_sizes(lengths, mk):
    """{(tid, tile of the contig): intervals of the pair} -- an interval is filed under every tile it covers a position of, "-1 at L - 1"
    under the last position's tile, and a pair is the RANGE of the sample's interval list from the first to the last one filed under
    the tile: what lies between is handed to the kernel too (it leaves the tile alone), and counts for the form the kernel takes."""
    first, last = {}, {}
    for tid, (_, _, ivs) in mk.items():
        for i, (b, e) in enumerate(ivs):
            lo, hi = ((e // TILE, e // TILE) if b > e else (b // TILE, (e - 1) // TILE))
            for t in range(lo, hi + 1):
                first.setdefault((tid, t), i)
                last[(tid, t)] = i
    return {k: last[k] - first[k] + 1 for k in first}


# ---- what qaCompute prints of the accumulators
def detail_text(names, lengths, acc, max_cov):
    out = []
    for c, name in enumerate(names):
        cum = [int(acc[c, 1 + k:2 + max_cov].sum()) for k in range(1, max_cov + 1)]
        out.append("%s\t%d\t" % (name, lengths[c]) + "".join("%d\t" % x for x in cum) + "\n")
    return "".join(out)


def avg_rows(names, lengths, acc):
    return ["%s\t%d\t%3.5f" % (n, L, float(int(acc[c, 0])) / L) for c, (n, L) in enumerate(zip(names, lengths))]


def covx_counts(acc, max_cov):
    return [int(acc[:, 1 + i:2 + max_cov].sum()) for i in range(1, max_cov + 1)]


def parse_cov_text(text, n_contigs, max_cov):
    """(contig rows, base counts of the Cov*X block) of a .cov file."""
    lines = text.split("\n")
    assert lines[0] == "Chromosome\tSeq_lem\tAvg_Cov" and lines[n_contigs + 2] == "Cov*X\tPercentage\tNr. of bases"
    return lines[1:1 + n_contigs], [int(l.split("\t")[2]) for l in lines[n_contigs + 3:n_contigs + 3 + max_cov]]


# ------------------------------------------------------------------------------------------------ the record sets
@functools.lru_cache(maxsize=None)
def rec(tid, pos, cigar, mapq=60, flag=0):
    qlen = sum(n for n, op in bt.parse_cigar(cigar) if op in (0, 1, 4, 7, 8))
    return bt.make_record(tid, pos, cigar, "A" * qlen, mapq=mapq, flag=flag)


def stream(reads):
    """reads: (tid, pos, cigar[, mapq[, flag]]) tuples -> the sample's record stream, sorted by (tid, pos)."""
    return np.frombuffer(b"".join(rec(*r) for r in sorted(reads, key=lambda r: (r[0], r[1]))), dtype=np.uint8)


def spread(tid, n, lo=10, hi=1990, mean_depth=5.0, salt=1):
    """n one-interval reads with starts spread over indices [lo, hi) of a tile and lengths 1 .. M, M sized for the mean depth: the
    depth wanders over many bins and falls back to 0 where the starts leave gaps."""
    m = max(2, int(2.0 * mean_depth * (hi - lo) / max(n, 1)))
    m = min(m, 400)
    out = []
    for i in range(n):
        idx = lo + (i * (hi - lo)) // n
        ln = 1 + (i * 2654435761 + salt * 40503) % m
        out.append((tid, idx - 1, "%dM" % ln))
    return out


class Case:
    def __init__(self, name, names, lengths, samples, cov_max=10, pairs=None, items=None, seqs=None):
        self.name, self.names, self.lengths, self.samples, self.cov_max = name, names, lengths, samples, cov_max
        self.pairs = pairs or {}          # {(sample, tid, tile of the contig): intervals} the case was built for
        self.items = items or {}          # {(tid, tile of the contig): [[samples of a work item], ...]} under the default knobs
        self.seqs = seqs
        self._mk = None

    def model(self, max_cov=None, min_mapq=1):
        """[sample][contig][17] and {(sample, tid, tile): intervals}; the difference arrays are walked once per case."""
        if self._mk is None:
            mk = [marks(self.lengths, s, min_mapq) for s in self.samples]
            self._mk = (mk, [depths(self.lengths, m) for m in mk])
        mk, dp = self._mk
        acc = np.stack([accumulators(self.lengths, d, self.cov_max if max_cov is None else max_cov) for d in dp])
        sizes = {(s, t, k): n for s, m in enumerate(mk) for (t, k), n in pair_sizes(self.lengths, m).items()}
        return acc, sizes

    def depth_never_negative(self, s, tid):
        d = self._mk[1][s].get(tid)
        return d is not None and bool(d.any()) and int(d.min()) >= 0


A_COUNTS = [1, 2, 63, 64, 65, 66, 67, 68, 255, 256, 257, 258, 259, 260, 511, 512, 513, 769]


def group_a():
    """One tile, one sample per interval count: one interval per lane up to 64, four per lane up to 256, steps of 256 beyond.  The
    dataset's last pair takes 769 (1 mod 4), 258 (2 mod 4) and 259 (3 mod 4) intervals in turn: the 16-byte loads behind its last
    interval land on the four {0, 0} entries that close the interval list."""
    out = []
    for last in (769, 258, 259):
        counts = [n for n in A_COUNTS if n != last] + [last]
        samples = [stream(spread(0, n, mean_depth=3.0 + (i % 5) * 2.5, salt=i)) for i, n in enumerate(counts)]
        out.append(Case("a_last%d" % last, ["a0"], [TILE], samples, cov_max=15, pairs={(i, 0, 0): n for i, n in enumerate(counts)},
                        items={(0, 0): [list(range(k, min(k + 4, len(counts)))) for k in range(0, len(counts), 4)]}))
    return out


def group_b():
    """The 16-bit half-words: piles of 32 767 intervals in the middle tile of a contig of three (one more = the wide variant by
    itself), an ordinary sample before the pile in its work item and one behind it."""
    L = 3 * TILE
    t1 = TILE
    shapes = {
        "even": lambda n: [(0, t1 + 100 - 1, "5M")] * n,
        "odd": lambda n: [(0, t1 + 101 - 1, "5M")] * n,
        "one_m_in_a_word": lambda n: [(0, t1 + 100 - 1, "1M")] * n,             # +n at 100, -n at 101: the halves of one word
        "one_m_over_two_words": lambda n: [(0, t1 + 101 - 1, "1M")] * n,        # +n at 101, -n at 102: two words
        "one_end": lambda n: [(0, t1 + 200 + i % 150 - 1, "%dM" % (200 - i % 150)) for i in range(n)],      # all end at 400
    }
    ordinary = lambda salt: [(0, p + t1, c) for (_, p, c) in spread(0, 40, 50, 600, 4.0, salt)] + [(0, 500, "30M"), (0, 2 * TILE + 700, "30M")]
    out = []
    for n in (32767, 32768):
        for tag, f in shapes.items():
            pile = f(n) + [(0, 300, "20M"), (0, 2 * TILE + 300, "20M")]           # ordinary reads of the pile's sample, in the other tiles
            out.append(Case("b_%s_%d" % (tag, n), ["b0"], [L], [stream(ordinary(1)), stream(pile), stream(ordinary(2))],
                            pairs={(1, 0, 1): n, (0, 0, 1): 40, (2, 0, 1): 40}, items={(0, 1): [[0, 1], [2]]}))
    pile = shapes["even"](32766) + [(0, t1 - 50, "100M")]                          # 32 766 and one interval that enters from the tile before
    out.append(Case("b_entering_32767", ["b0"], [L], [stream(ordinary(1)), stream(pile), stream(ordinary(2))],
                    pairs={(1, 0, 1): 32767, (1, 0, 0): 1}, items={(0, 1): [[0, 1], [2]]}))
    return out


C_DEPTHS = list(range(1, 16)) + [40]


def group_c():
    """Histogram fields: the middle tile of contig 0 at one depth over all 2048 positions (every lane adds 32 to one byte field, four
    lanes reach 128, the bin reaches 2048), sample d at depth d; a tile with one interval of 5 bases; a tile whose halves sit at
    depths 7 and 8, the two byte-field registers."""
    names, lengths = ["c_flat", "c_five", "c_halves"], [3 * TILE, TILE, 3 * TILE]
    samples = [stream([(0, 1000, "4000M")] * d) for d in C_DEPTHS]
    samples.append(stream([(1, 700, "5M")]))
    samples.append(stream([(2, 1000, "4000M")] * 7 + [(2, TILE + 1024 - 1, "2500M")]))
    pairs = {(i, 0, 1): d for i, d in enumerate(C_DEPTHS)}
    pairs.update({(16, 1, 0): 1, (17, 2, 1): 8})
    return [Case("c_max%d" % m, names, lengths, samples, cov_max=m, pairs=pairs) for m in (15, 10, 1)]


D_BREAKS = [0, 1, 31, 32, 33, 63, 64, 2015, 2016, 2046, 2047]
D_LENGTHS = [1, 2, 31, 32, 33, 2047, 2048, 2049, 4097]


def group_d():
    """Lane and tile edges.  d_breaks: starts and ends on the first and last indices of lanes 0, 1 and 63 of a middle tile, an end on
    the tile's last index and one on the next tile's index 0, a start on index 2047 that crosses two seams by N / D operations, a
    read at pos 0.  d_ends: contigs of 1 .. 4097 bases with reads up to, onto and over their ends -- the clamp onto L - 1, the cursor
    at and beyond L, last tiles of 1, 31, 32 and 33 scanned positions."""
    reads = [(0, 0, "3M")]
    for k in D_BREAKS:
        reads.append((0, TILE + k - 1, "2M"))                                 # starts on k
        reads.append((0, TILE + k - 7 - 1, "7M"))                             # ends on k (k = 0: in the tile before, its -1 on this tile's index 0)
    reads += [(0, 2 * TILE - 9 - 1, "9M"), (0, 2 * TILE - 30 - 1, "29M")]    # -1 on the next tile's index 0; on this tile's last index
    reads += [(0, 2047 - 1, "1M2100N3M"), (0, 2047 - 1, "1M4200D3M"), (0, 2047 - 1, "4300M")]
    s1 = spread(0, 90, 10, 4 * TILE, 3.0, 3)
    breaks = Case("d_breaks", ["d0"], [5 * TILE], [stream(reads), stream(s1)], cov_max=15, pairs={(0, 0, 1): 28})
    r0, r1 = [], []
    for c, L in enumerate(D_LENGTHS):
        r0 += [(c, 0, "1M"), (c, L - 1, "1M"), (c, max(0, L - 20), "30M"), (c, max(0, L - 5), "2M8I2M"), (c, 0, "%dM" % L)]
        if L >= 2:
            r0.append((c, L - 2, "1M"))                                        # +1 and -1 both on L - 1: nothing
        if L >= 31:
            r0 += [(c, L - 31, "10M"), (c, L - 12, "4S11M"), (c, L - 30, "40M", 0), (c, L - 30, "40M", 60, 0x400)]
        if L >= 2047:
            r1 += spread(c, 30, 5, L - 5, 2.0, c) + [(c, L - 1, "1M4S")]
    ends = Case("d_ends", ["d%d" % L for L in D_LENGTHS], D_LENGTHS, [stream(r0), stream(r1)], cov_max=15)
    return [breaks, ends]


E_CARRIED = [1, 3, 4, 5, 8, 9]
E_ROT = [20, 300, 64, 65]


def group_e():
    """Work items: tiles carried by 1, 3, 4, 5, 8 and 9 samples (items of at most four pairs), then four tiles in which samples 0-3
    hold 20, 300, 64 and 65 intervals in every rotation -- the three forms of the scatter side by side in one wavefront's loop.  Sample
    9 is empty, every read of sample 10 is below cov_min_mapq; most samples are absent from most contigs."""
    n_c = len(E_CARRIED) + len(E_ROT)
    reads = [[] for _ in range(11)]
    pairs, items = {}, {}
    for c, k in enumerate(E_CARRIED):
        for s in range(k):
            n = 7 + 5 * ((s + c) % 4)
            reads[s] += spread(c, n, 10 + 100 * s, 1900, 2.0 + s, s + c)
            pairs[(s, c, 0)] = n
        items[(c, 0)] = [list(range(j, min(j + 4, k))) for j in range(0, k, 4)]
    for j in range(len(E_ROT)):
        c = len(E_CARRIED) + j
        for s in range(4):
            n = E_ROT[(s + j) % 4]
            reads[s] += spread(c, n, 10 + 37 * s, 2000, 4.0 + s, s + j)
            pairs[(s, c, 0)] = n
        items[(c, 0)] = [[0, 1, 2, 3]]
    reads[10] = [(0, p, cg, 0) for (_, p, cg) in spread(0, 25, 10, 1900, 3.0, 9)]
    return [Case("e_items", ["e%d" % c for c in range(n_c)], [TILE] * n_c, [stream(r) for r in reads], cov_max=10, pairs=pairs, items=items)]


def group_f():
    """Accumulator copies: a contig of 17 tiles and one of 9 (tile % 8 wraps), sparse reads in every tile, some over a seam; with a
    reference sequence, so that the fused run takes the same index."""
    lengths = [17 * TILE - 100, 9 * TILE - 1]
    samples = []
    for s in range(3):
        r = []
        for c, L in enumerate(lengths):
            for t in range((L + TILE - 1) // TILE):
                for j in range(3 + (t + s) % 4):
                    idx = t * TILE + 40 + (577 * j + 131 * s + 29 * t) % 1900
                    ln = 20 + (j * 37 + t * 11 + s * 5) % 200
                    if idx + ln < L:
                        r.append((c, idx - 1, "%dM" % ln))
        samples.append(stream(r))
    return [Case("f_copies", ["f17", "f9"], lengths, samples, cov_max=15, seqs=["A" * L for L in lengths])]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}, built once per process."""
    return {c.name: c for g in (group_a, group_b, group_c, group_d, group_e, group_f) for c in g()}


CASE_NAMES = (["a_last%d" % n for n in (769, 258, 259)]
              + ["b_%s_%d" % (t, n) for n in (32767, 32768) for t in ("even", "odd", "one_m_in_a_word", "one_m_over_two_words", "one_end")]
              + ["b_entering_32767"] + ["c_max%d" % m for m in (15, 10, 1)] + ["d_breaks", "d_ends", "e_items", "f_copies"])
