"""Inputs that put the device per-read stage (csrc/devpack.hip: piece_lane, low_flags8, tweak_pair, msnv_token_clamp) at the seams of
quality bytes and of piece geometry, built with bamtools.make_record and nothing else (no GPU, no library call): the GPU tests
(tests/test_gpu_piece_seams.py) send them through packsame._same_dataset, the CPU tests (tests/test_piececases_model.py) check that the
cases hold what they claim and that a closed-form model gives the oracle's calls on them.

The layout rule every family follows: msnv_emit_block takes its LDS-image route only for a block of 64 CONSECUTIVE records of the round
that belong to ONE sample, total 20 480 bytes or less, whose seq stretch fits EO_BYTES, with at most EQ_CAP further pieces and no record
that opens with the `<l_seq>S` placeholder -- so every seam sample holds a multiple of 64 records (a case of one read per sample would
send everything to msnv_emit_block_slow and test nothing of the image form).  Reads of a seam sample lie at disjoint reference
positions, the reference there is one letter and the reads another: a position's count in the called text is exactly one base's flag."""
import bamtools as bt

TILE, SEG_MAX, PB = 2048, 128, 64                      # include/msnv.h: positions per tile, bases per piece; devpack.hip: records per block
EW_BYTES, EO_BYTES, EQ_CAP, OVL_SLOTS = 20480, 6144, 32, 8

Q_FLAG = (0, 1, 12, 13, 14, 63, 64, 65, 126, 127, 128, 129, 199, 200, 201, 253, 254, 255)
# 16 / 17, 79 / 80, 158 / 159: 0.8 x truncates to 12 / 13, 63 / 64, 126 / 127 -- next to a cutoff behind the edit of disagreeing mates
Q_OVL = (0, 1, 12, 13, 16, 17, 63, 64, 79, 80, 81, 100, 126, 127, 128, 158, 159, 160, 199, 200, 201, 254, 255)
CUTOFFS_ORACLE = (0, 1, 13, 64, 127)
CUTOFFS_HOST_ONLY = (128, 255)                         # min_baseq above 127 flags every base (all_low) whatever is stored: outside the oracle's domain
PIECE_LEN = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257)
EDGE_BEFORE = (1, 2, 3, 4, 5, 31, 32, 33)              # family B: a read of 40 bases starts this far in front of a tile edge
EDGE_END = ((1, 39), (2, 38), (3, 37), (4, 37), (1, 37), (3, 39), (0, 39), (2, 37))      # ... and a read of `len` bases ends this far in front of one
BASES_ORACLE = "=ACGTN"                                # the codes the reference snpCall takes; it dereferences an empty vector at the other ten
E_QUALS = (126, 127, 128, 200, 254, 255)               # 254 = 0xfe, the host stage's QUAL_CUT mark


class Case(tuple):
    """(names, lengths, seqs, samples) -- what packsame._same_dataset and parity.run_oracle take -- with what the builder knows about
    the case in .meta."""
    def __new__(cls, names, lengths, seqs, samples, **meta):
        self = super().__new__(cls, (names, lengths, seqs, samples))
        self.meta = meta
        return self


def _name(k, n_chars):
    """A name of n_chars characters, another one for every k < 62 ** n_chars."""
    abc = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    s = ""
    for _ in range(n_chars):
        s = abc[k % 62] + s
        k //= 62
    assert k == 0
    return s


def _fit(cur, span, blocked=()):
    """The first position >= cur where `span` reference positions cross no tile edge and touch no blocked interval."""
    moved = True
    while moved:
        moved = False
        edge = (cur // TILE + 1) * TILE
        if cur + span > edge:
            cur, moved = edge, True                    # (a read that STARTS on an edge is fine: nothing of it lies in the tile before)
        for lo, hi in blocked:
            if cur < hi and cur + span > lo:
                cur, moved = hi, True
    return cur


def _stream(recs):
    """(pos, record) pairs -> one stream in file order (sorted by position, stable)."""
    return bt.records(*[r for _, r in sorted(recs, key=lambda t: t[0])])


def ref_span(cigar):
    return sum(n for n, op in bt.parse_cigar(cigar) if op in (0, 2, 3, 7, 8))


def pieces(stream):
    """The pieces the per-read stage cuts from a stream of pileup reads, in file order: (tile-global position, bases).  Every aligned block
    (M, =, X) is cut at SEG_MAX bases and at every tile edge (devpack.hip: emit_walk; pack.cpp: pack_sample)."""
    out = []
    for r in bt.iter_records(stream):
        rp = r["pos"]
        for l, op in r["cigar"]:
            if op in (0, 7, 8):
                off = 0
                while off < l:
                    g = rp + off
                    n = min(SEG_MAX, l - off, TILE - g % TILE)
                    out.append((g, n))
                    off += n
                rp += l
            elif op in (2, 3):
                rp += l
    return out


def record_offsets(stream):
    """Per record of a stream: (offset of the record, of its SEQ field, of its QUAL field, its size)."""
    import struct
    buf, off, out = bytes(stream), 0, []
    while off < len(buf):
        bs = struct.unpack_from("<i", buf, off)[0]
        l_name = buf[off + 12]
        n_cig = struct.unpack_from("<H", buf, off + 16)[0]
        l_seq = struct.unpack_from("<i", buf, off + 20)[0]
        seq_o = off + 36 + l_name + 4 * n_cig
        out.append((off, seq_o, seq_o + (l_seq + 1) // 2, bs + 4))
        off += bs + 4
    return out


# ---------------------------------------------------------------------------------- family A: quality flags
def family_a():
    """Two samples of 64 and 128 reads of 128 bases, all C over a reference of A, at disjoint positions.  Qualities: Q_FLAG rotated by one
    more byte for every ramp read, so every value lands in every one of the 8 byte slots of a low_flags8 word and in each of the four
    lanes; one read in eight is all 0xff (a BAM written without qualities), one is all 0.  Names of 1, 2, 3 and 4 characters cycle and
    every third read carries aux fields: the SEQ and QUAL fields start at every byte offset mod 4 (the alignbyte loads).  The round's
    last record carries no aux bytes.  meta: reads[s] = [(pos, quals)]."""
    n_reads, rlen, samples, meta_reads = (64, 128), 128, [], []
    L = 16 + 130 * max(n_reads) + 64
    for s, n in enumerate(n_reads):
        recs, reads, ramp = [], [], 0
        for k in range(n):
            if k % 8 == 3:
                q = [255] * rlen
            elif k % 8 == 7:
                q = [0] * rlen
            else:
                q = [Q_FLAG[(j + ramp) % len(Q_FLAG)] for j in range(rlen)]
                ramp += 1
            pos = 16 + 130 * k + s                     # (the two samples' reads start one position apart: every read crosses 8-base and 32-base boundaries differently)
            last = s == len(n_reads) - 1 and k == n - 1
            aux = bt.aux_fields(nm=k % 7, md="128", score=100 + k) if k % 3 == 0 and not last else b""
            recs.append((pos, bt.make_record(0, pos, "%dM" % rlen, "C" * rlen, qual=q, name=_name(k // 4, k % 4 + 1), aux=aux)))
            reads.append((pos, q))
        samples.append(_stream(recs))
        meta_reads.append(reads)
    return Case(["qa"], [L], ["A" * L], samples, reads=meta_reads, read_len=rlen)


# ---------------------------------------------------------------------------------- family B: piece lengths and cuts
def family_b(short_fasta=True):
    """One sample.  A read for every value of PIECE_LEN, once as nM and once as 1SnM (odd first base: the q0 & 1 funnel); reads of 40 bases
    that start EDGE_BEFORE positions in front of a tile edge (cut there); reads that END 0 to 4 positions in front of one with lengths
    that are no multiple of 4 (pad_in_tile 0 to 3, n_pad 1 to 3); a read over the contig's end, and -- short_fasta -- on a second contig one over the
    end of a FASTA record 100 characters shorter than its contig.  Padded to a multiple of 64 with plain reads.  Reads C over a reference of A,
    qualities 13, 12 alternating: every base's flag differs from its neighbour's.  meta: n_pieces, edge_before, pad_in_tile, lens."""
    fixed, blocked = [], []
    qual = lambda n: [13 - (j & 1) for j in range(n)]
    rec = lambda pos, cigar, n, name: (pos, bt.make_record(0, pos, cigar, "C" * n, qual=qual(n), name=name))
    edge, crossing, pads = TILE, {}, set()
    for d in EDGE_BEFORE:
        fixed.append(rec(edge - d, "40M", 40, "x%d" % d))
        blocked.append((edge - d - 2, edge - d + 42))
        crossing[edge] = d
        edge += TILE
    for e, n in EDGE_END:                              # shares an edge with a crossing read that starts at or behind its end (d <= e), else takes one of its own
        at = max((g for g, d in crossing.items() if d <= e), key=lambda g: crossing[g], default=None)
        if at is None:
            at, edge = edge, edge + TILE
        else:
            del crossing[at]
        fixed.append(rec(at - e - n, "%dM" % n, n, "e%d_%d" % (e, n)))
        blocked.append((at - e - n - 2, at - e + 2 if e else at + 2))
        pads.add((min(e, 3), n))
    recs, cur, lens = list(fixed), 8, []
    for n in PIECE_LEN:
        for clip in (0, 1):
            cur = _fit(cur, n, blocked)
            cigar = "%dM" % n if not clip else "1S%dM" % n
            recs.append((cur, bt.make_record(0, cur, cigar, "G" * clip + "C" * n, qual=[40] * clip + qual(n), name="p%d_%d" % (n, clip))))
            lens.append((n, clip))
            cur += n + 3
    L = max(edge, (cur // TILE + 1) * TILE) + 300      # the contig ends inside a tile
    recs.append(rec(L - 20, "40M", 40, "overC"))       # over the contig's end
    blocked.append((L - 22, L + 22))
    tail = []
    if short_fasta:                                    # a second contig whose FASTA record is 100 characters shorter than the contig (a read that STARTS behind the record's end is no pileup read)
        tail = [(0, bt.make_record(1, 10, "30M", "C" * 30, qual=qual(30), name="s0")), (1, bt.make_record(1, 280, "40M", "C" * 40, qual=qual(40), name="overF"))]
    k = 0
    while (len(recs) + len(tail)) % PB:
        cur = _fit(cur, 30, blocked)
        recs.append(rec(cur, "30M", 30, "f%d" % k))
        cur += 33; k += 1
    assert cur + 40 < L - 22
    stream = bt.records(*[r for _, r in sorted(recs, key=lambda t: t[0])] + [r for _, r in tail])
    names, lengths, seqs = ["pb"], [L], ["A" * L]
    if short_fasta:
        names, lengths, seqs = names + ["pbs"], lengths + [400], seqs + ["A" * 300]
    return Case(names, lengths, seqs, [stream], n_pieces=len(pieces(stream)), pad_in_tile=sorted(pads), lens=lens)


# ---------------------------------------------------------------------------------- family C: base codes
def family_c(codes=BASES_ORACLE):
    """One sample of 64 reads whose bases run through `codes`, rotated by one for every read, over a reference that runs through
    A C G T N a c g t n: every code at every nibble slot 0 to 31 of a lane at both parities of the first base (nM and 1SnM alternate), `=`
    over a known letter, over N and over a lower-case letter.  The pieces whose mismatches are sampled (every 16th of the sample) include
    one shorter than 16 bases and one of 17 to 31.  codes = BASES_ORACLE: what the oracle takes (C1);
    codes = bamtools.NT16: all sixteen (C2, device against host only).  meta: sampled (lengths of the sampled pieces)."""
    long_, short = (40, 64, 33, 32, 45, 96, 37, 50), (9, 15, 16, 17, 31, 23, 21, 12, 5, 29, 3, 27, 19, 1, 30, 8)
    recs, cur = [], 11
    for k in range(64):
        # reads 0 .. 31: a lane's 32 nibbles and more, every rotation at both parities; reads 32 .. 63: short ones (reads 32 and 48 are sampled: 9 and 23 bases)
        n = long_[k % 8] if k < 32 else short[(k - 32 + 5 * ((k - 32) // 16)) % 16]
        clip, rot = k & 1, k // 2
        cur = _fit(cur, n)
        seq = "".join(codes[(j + rot) % len(codes)] for j in range(n))
        recs.append((cur, bt.make_record(0, cur, "%dM" % n if not clip else "1S%dM" % n, "A" * clip + seq, qual=[30] * clip + [13 - (j & 1) for j in range(n)], name="c%d" % k)))
        cur += n + 1 + k % 3
    L = cur + 50
    ref = ("ACGTNacgtn" * (L // 10 + 1))[:L]
    stream = _stream(recs)
    pc = pieces(stream)
    return Case(["pc"], [L], [ref], [stream], sampled=[n for _, n in pc[::16]], n_pieces=len(pc), codes=codes)


# ---------------------------------------------------------------------------------- family D: overlapping mates
def _pair(pos, name, n, b1, b2, q1, q2, cigar1=None):
    c1 = cigar1 or "%dM" % n
    return [(pos, bt.make_record(0, pos, c1, b1 * n, qual=q1, flag=99, name=name, mtid=0, mpos=pos, tlen=max(n, ref_span(c1)))),
            (pos, bt.make_record(0, pos, "%dM" % n, b2 * n, qual=q2, flag=147, name=name, mtid=0, mpos=pos, tlen=-max(n, ref_span(c1))))]


def family_d():
    """Sample 0: fully overlapping proper pairs (flags 99 / 147) of 23 bases a mate over a reference of A.  Pair i has the first mate's
    quality constant at Q_OVL[i] and the second mate's running through Q_OVL: every (x, y).  Once with agreeing bases (C, C), once with
    disagreeing ones (C, G), and both again with the first mate 10M2D13M (the cursor skips).  Plain reads between the pairs pad the sample
    to 192 records.  Sample 1: a pair whose mates are both all 0xff, a pair in which one mate has SEQ *, a group of exactly OVL_SLOTS
    alignments under one name, plain reads up to 64 records.  meta: pair_pos[(kind, form, i)] = position of pair i's first base."""
    nq = len(Q_OVL)
    recs, pair_pos, cur, k = [(4, bt.make_record(0, 4, "8M", "A" * 8, name="first"))], {}, 20, 0      # (snpCall drops the first line of the text: it is this read's)
    plain = lambda pos, nm: (pos, bt.make_record(0, pos, "12M", "C" * 12, qual=[13 - (j & 1) for j in range(12)], name=nm))
    for form, cigar1 in (("plain", None), ("del", "10M2D13M")):
        for kind, b2 in (("agree", "C"), ("differ", "G")):
            for i in range(nq):
                cur = _fit(cur, nq + 2)
                recs += _pair(cur, "%s%s%d" % (form[0], kind[0], i), nq, "C", b2, [Q_OVL[i]] * nq, list(Q_OVL), cigar1)
                pair_pos[(kind, form, i)] = cur
                cur += nq + 4
                if i % 12 == 5 and k < 7:
                    cur = _fit(cur, 12)
                    recs.append(plain(cur, "s%d" % k)); k += 1; cur += 14
    assert len(recs) == 4 * 2 * nq + 8 and len(recs) % PB == 0
    L0 = cur
    # sample 1
    r1 = [(4, bt.make_record(0, 4, "8M", "A" * 8, name="first"))]
    r1 += _pair(30, "ff", 23, "C", "C", [255] * 23, [255] * 23)
    r1 += [(70, bt.make_record(0, 70, "23M", "C" * 23, qual=[30] * 23, flag=99, name="ns", mtid=0, mpos=70, tlen=23)),
           (70, bt.make_record(0, 70, "23M", "*", flag=147, name="ns", mtid=0, mpos=70, tlen=-23))]
    for m in range(OVL_SLOTS):                         # eight alignments of one template, each overlapping the next and naming it as its mate: four edited pairs
        r1.append((110 + 5 * m, bt.make_record(0, 110 + 5 * m, "20M", "C" * 20, qual=[Q_OVL[(3 * m + j) % nq] for j in range(20)], flag=99 if m % 2 == 0 else 147,
                                               name="tmpl", mtid=0, mpos=115 + 5 * m, tlen=25)))
    c1, k = 200, 0
    while len(r1) % PB:
        r1.append(plain(c1, "t%d" % k)); c1 += 15; k += 1
    L = (max(L0, c1) // 64 + 2) * 64
    return Case(["pd"], [L], ["A" * L], [_stream(recs), _stream(r1)], pair_pos=pair_pos, n_q=nq)


# ---------------------------------------------------------------------------------- family E: the token mark against stored bit-7 qualities
def family_e(stack=128):
    """One round, two samples from the same 64 reads (20 bases of C over A at disjoint positions, qualities E_QUALS rotated).  Sample 0 is
    shallow: no clamp, no marks -- its bases of quality 128 / 254 / 255 are counted as stored.  Sample 1 adds `stack` reads that start at
    ONE position (3 characters per read start): with a token_limit of 300 the reads behind the 100th are cut at that position, so
    msnv_token_clamp and msnv_token_cut run on the sample.  meta: shared = [(pos, quals)], stack_pos, stack_len, stack_quals."""
    shared, recs0, cur = [], [], 10
    for k in range(64):
        q = [E_QUALS[(j + k) % len(E_QUALS)] for j in range(20)]
        cur = _fit(cur, 20)
        recs0.append((cur, bt.make_record(0, cur, "20M", "A" * 20 if k == 0 else "C" * 20, qual=q, name="e%d" % k)))      # (read 0 matches: the dropped first line is no call)
        shared.append((cur, q))
        cur += 22
    p0 = cur + 10
    recs1, sq = list(recs0), []
    for k in range(stack):
        q = [E_QUALS[(j + k) % len(E_QUALS)] for j in range(16)]
        recs1.append((p0, bt.make_record(0, p0, "16M", "C" * 16, qual=q, name="k%d" % k)))
        sq.append(q)
    assert len(recs1) % PB == 0
    L = p0 + 100
    return Case(["pe"], [L], ["A" * L], [_stream(recs0), _stream(recs1)], shared=shared, stack_pos=p0, stack_len=16, stack_quals=sq, token_limit=300)


def d_position(case, kind, x, y, form="plain"):
    """Family D: the 0-based position where a first mate's base of quality x meets a second mate's of quality y (kind: agree / differ)."""
    return case.meta["pair_pos"][(kind, form, Q_OVL.index(x))] + Q_OVL.index(y)


def calls_at(text):
    """called_SNPs text -> {0-based position: (coverage per sample, {allele: counts per sample})}."""
    out = {}
    for line in text.split("\n"):
        if not line:
            continue
        w = line.split("\t")
        alleles = {}
        for a in w[5].split(","):
            f = a.split("|")
            alleles[f[1]] = [int(v) for v in f[3:]]
        out[int(w[2]) - 1] = ([int(v) for v in w[4].split("|")], alleles)
    return out
