"""Hand-placed record streams for tests/test_gpu_record_walk.py: every record's offset is chosen against the seams of the device pack's
record walk (csrc/devrec.h: a stream is cut into sub-segments of MSNV_SCAN_SUB bytes counted from its first byte).  A builder places
the records, then asserts in plain Python the property its case is named for -- a fixture that drifts fails here, on the CPU, before
anything touches the device (tests/test_record_walk_fixtures.py runs every builder)."""
import random
import types

import numpy as np

import bamtools as bt


def _ref(n, seed):
    rnd = random.Random(seed)
    return "".join(rnd.choice("ACGT") for _ in range(n))


REF0, REF1 = _ref(6000, 11), _ref(6000, 12)
NAMES, LENGTHS, SEQS = ["c0", "c1"], [6000, 6000], [REF0, REF1]
DEFAULT_SUB = 6144                    # knobs.h: SCAN_SUB_ROUND
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def cap2(sub):
    """Slots per sub-segment of the quick walk (devpack.hip: Round::stage)."""
    return sub // 48 + 2


def seq_for(ref, pos, cigar):
    out, p = [], pos
    for n, op in bt.parse_cigar(cigar):
        if op in (0, 7, 8):
            out.append(ref[p:p + n]); p += n
        elif op in (2, 3):
            p += n
        elif op in (1, 4):
            out.append("A" * n)
    return "".join(out)


def sized(size, tid, pos, cigar, seq, name, **kw):
    """A record of exactly `size` bytes: the read name grows by up to 196 characters, what is left goes into one aux field XX:Z."""
    base = len(bt.make_record(tid, pos, cigar, seq, name=name, **kw))
    pad = size - base
    assert pad >= 0, "a record of %d bytes cannot be made %d bytes long" % (base, size)
    aux = b""
    if pad > 200:
        aux = b"XXZ" + b"x" * (pad - 200) + b"\0"
        pad = 196
    r = bt.make_record(tid, pos, cigar, seq, name=name + "a" * pad, aux=aux, **kw)
    assert len(r) == size
    return r


class Stream:
    """Records one behind the other; starts[i] is record i's offset from the stream's first byte, kinds[i] what it is: "read" (enters the
    pileup), "filt" (mapped, a duplicate: no pileup read), "unm" (unmapped)."""

    def __init__(self, sub, tid=0, pos=20, step=3, refs=SEQS, tag="r", name_first=""):
        self.sub, self.tid, self.pos, self.step, self.refs, self.tag, self.name_first = sub or DEFAULT_SUB, tid, pos, step, refs, tag, name_first
        self.recs, self.starts, self.kinds, self.off = [], [], [], 0

    def _name(self):
        return "%s%s%d" % (self.name_first, self.tag, len(self.recs))

    def add(self, rec, kind):
        self.starts.append(self.off); self.recs.append(rec); self.kinds.append(kind); self.off += len(rec)
        return len(self.recs) - 1

    def read(self, size=None, n=30, cigar=None, seq=None, pos=None, tid=None, kind="read", name=None, **kw):
        """A mapped read at the next position (or at pos / on contig tid, where the stream then goes on)."""
        if tid is not None:
            self.tid = tid
        if pos is not None:
            self.pos = pos
        ref = self.refs[self.tid] if 0 <= self.tid < len(self.refs) else self.refs[0]
        if cigar is None:
            cigar = "%dM" % n
            if seq is None:
                seq = ref[self.pos:self.pos + n]
                if self.pos % 4 == 0 and n > 8:
                    seq = seq[:7] + OTHER[seq[7]] + seq[8:]              # (something to call)
        elif seq is None:
            seq = seq_for(ref, self.pos, cigar)
        if kind == "filt":
            kw["flag"] = 0x400
        name = self._name() if name is None else name
        base = bt.make_record(self.tid, self.pos, cigar, seq, name=name, **kw)
        rec = base if size is None else sized(size, self.tid, self.pos, cigar, seq, name, **kw)
        self.pos += self.step
        return self.add(rec, kind)

    def tiny(self, pos=None, cigar="1M", **kw):
        """The shortest mapped read: 44 bytes (two fit into a sub-segment of 64)."""
        if pos is not None:
            self.pos = pos
        r = bt.make_record(self.tid, self.pos, cigar, self.refs[self.tid][self.pos], name=self.name_first or "t", **kw)
        assert len(r) == 44
        self.pos += self.step
        return self.add(r, "read")

    def unm(self, size=37):
        assert size >= 37
        return self.add(sized(size, -1, -1, "*", "", self.name_first, flag=4), "unm")

    def min_size(self, kind):
        return 37 + len(self.name_first) if kind == "unm" else len(bt.make_record(0, 0, "30M", "A" * 30, name=self._name() + "00"))

    def fill_to(self, target, kind="read"):
        """Records of `kind` up to exactly `target` bytes of stream."""
        while self.off != target:
            gap, lo = target - self.off, self.min_size(kind)
            assert gap >= lo, "%d bytes cannot be filled with a %s record (%d at least)" % (gap, kind, lo)
            size = lo + 11 if gap >= 2 * lo + 24 else gap
            if kind == "unm":
                self.unm(size)
            else:
                self.read(size=size, kind=kind)
        return self

    def seam(self, d=0, kind="read", least=1):
        """The next seam index k such that records of `kind` can be filled up to k * sub - d (d bytes in front of the seam; negative: behind it)."""
        k = max(least, (self.off + d + self.sub - 1) // self.sub)
        while not (k * self.sub - d == self.off or k * self.sub - d - self.off >= self.min_size(kind) + 8):
            k += 1
        return k

    def sub_of(self, i):
        return self.starts[i] // self.sub

    def starts_in(self, k):
        return [i for i, s in enumerate(self.starts) if k * self.sub <= s < (k + 1) * self.sub]

    @property
    def n_sub(self):
        return max(1, (self.off + self.sub - 1) // self.sub)

    def bytes(self, cut=0):
        b = b"".join(self.recs)
        return np.frombuffer(b[:len(b) - cut] if cut else b, dtype=np.uint8)


def plain(sub=None, n=24, tag="p"):
    st = Stream(sub, pos=40, tag=tag)
    for _ in range(n):
        st.read()
    return st


def case(streams, sub=None, params=None, many=False, names=NAMES, lengths=LENGTHS, seqs=SEQS, **notes):
    """params: keyword arguments of core.default_params (None: min_coverage = calling_threshold = 1, so that a handful of reads is called)."""
    params = dict(min_coverage=1, calling_threshold=1) if params is None else params
    samples = [s.bytes() if isinstance(s, Stream) else s for s in streams]
    return types.SimpleNamespace(names=names, lengths=lengths, seqs=seqs, samples=samples, streams=streams, sub=sub, params=params, many=many, **notes)


EMPTY = np.zeros(0, np.uint8)

# ------------------------------------------------------------------------------------------------ A: where a record meets a seam


def a_seam_offsets(sub):
    """Records that start exactly on a seam and 1, 3, 4, 35, 36 bytes in front of one: the block_size word (4 bytes) or the fixed header
    (36 bytes) lies across it, or ends at it."""
    st = Stream(sub)
    st.read()
    for d in (0, 1, 3, 4, 35, 36):
        k = st.seam(d)
        st.fill_to(k * sub - d)
        i = st.read()
        assert st.starts[i] == k * sub - d and (d == 0 or st.sub_of(i) == k - 1)
    st.read(); st.read()
    return case([st, plain(sub)], sub)


def a_residues(sub):
    """The first record start of a sub-segment at each of the 16 residues mod 16 behind the seam (guess_entry reads aligned 16-byte pieces
    and tries the 16 offsets of each)."""
    st = Stream(sub)
    st.read()
    for r in range(16):
        k = st.seam(-r)
        st.fill_to(k * sub + r)
        i = st.read()
        assert st.starts[i] == k * sub + r and st.starts_in(k)[0] == i and st.starts[i - 1] < k * sub
    st.read(); st.read()
    assert {s % 16 for s in st.starts} == set(range(16))
    return case([st, plain(sub)], sub)


def a_long_records(sub):
    """A record longer than one sub-segment and one longer than three: whole sub-segments where nothing starts; the record's last byte is
    the last of a sub-segment, or the first of the next."""
    st = Stream(sub)
    st.read()
    for span, endmod in ((1, 0), (1, 1), (3, 0), (3, 1)):
        k = st.seam(-(sub // 8))
        st.fill_to(k * sub + sub // 8)
        end = (k + span + 1) * sub + endmod
        i = st.read(size=end - st.off)
        st.read()
        assert st.starts[i + 1] == end and len(st.recs[i]) > span * sub
        assert all(not st.starts_in(j) for j in range(k + 1, k + span + 1))
        assert (st.starts[i + 1] - 1) % sub == (sub - 1 if endmod == 0 else 0)
    st.read()
    return case([st, plain(sub)], sub)


def a_tails(sub):
    """Streams whose length is a multiple of the sub-segment, and whose last sub-segment is 1, 35 and 36 bytes long (no header fits in it)."""
    out = []
    for t in (0, 1, 35, 36):
        st = Stream(sub, tag="t%d" % t)
        st.read(); st.read()
        k = st.seam(-t, least=3)
        st.fill_to(k * sub + t)
        assert st.off % sub == t and st.n_sub == k + (1 if t else 0)
        out.append(st)
    return case(out + [plain(sub)], sub)


def a_ends(sub):
    """The first record of a sub-segment is the last, or the second to last, of its stream (the guess asks for two successors); a stream of
    one record; empty streams first, last and in between -- one round."""
    a = Stream(sub, tag="a"); a.read()
    k = a.seam(-5, least=2); a.fill_to(k * sub + 5); i = a.read()
    assert a.starts_in(k)[0] == i == len(a.recs) - 1
    b = Stream(sub, tag="b"); b.read()
    k = b.seam(-5, least=2); b.fill_to(k * sub + 5); i = b.read(); b.read()
    assert b.starts_in(k)[0] == i == len(b.recs) - 2
    one = Stream(sub, tag="o"); one.read()
    assert len(one.recs) == 1
    streams = [EMPTY, one, a, EMPTY, b, plain(sub), EMPTY]
    assert streams[0].size == 0 and streams[3].size == 0 and streams[-1].size == 0
    return case(streams, sub, many=True)


A_CASES = [a_seam_offsets, a_residues, a_long_records, a_tails, a_ends]

# ------------------------------------------------------------------------------------------------ B: slot limits


def b_cap2(over):
    """MSNV_SCAN_SUB=480: cap2 = 12 slots.  Twelve unmapped records of 40 bytes fill a sub-segment to exactly 12 record starts; thirteen of
    37 bytes make 13 starts in one sub-segment.  Mapped reads in front and behind."""
    sub = 480
    assert cap2(sub) == 12
    st = Stream(sub)
    st.read()
    k = st.seam(0)
    st.fill_to(k * sub)
    for _ in range(13 if over else 12):
        st.unm(37 if over else 40)
    for _ in range(8):
        st.read()
    most = max(len(st.starts_in(j)) for j in range(st.n_sub))
    assert len(st.starts_in(k)) == most == (13 if over else 12)
    if not over:
        assert st.starts_in(k + 1)[0] == st.starts_in(k)[-1] + 1 and st.starts[st.starts_in(k + 1)[0]] == (k + 1) * sub
    return case([st, plain(sub)], sub)


def b_unmapped_tail():
    """No knob: an ordinary sample that ends in 400 unmapped records of 37 bytes -- 167 starts in a sub-segment of 6144 bytes, 130 slots."""
    st = Stream(None, step=2)
    for _ in range(60):
        st.read()
    for _ in range(400):
        st.unm(37)
    assert max(len(st.starts_in(j)) for j in range(st.n_sub)) > cap2(DEFAULT_SUB) == 130
    return case([st, plain()], None)


BIG_LEN = 150000


def b_field_overflow():
    """SubInfo.flags & 8: SEQ-less reads of 140000M, and two of 70000M that start in one sub-segment, under -Q 0: the places inside the
    sub-segment (seq bytes, pieces) pass 16 bits.  MSNV_SCAN_SUB=8192 (the quick route is still tried)."""
    sub = 8192
    ref = _ref(BIG_LEN, 13)
    a = Stream(sub, refs=[ref], pos=100, tag="a")
    a.read(); a.read(cigar="140000M", seq="*", pos=500); a.read(pos=600)
    b = Stream(sub, refs=[ref], pos=100, tag="b")
    b.read(); i = b.read(cigar="70000M", seq="*", pos=500); j = b.read(cigar="70000M", seq="*", pos=900); b.read(pos=1000)
    assert b.sub_of(i) == b.sub_of(j) and 70000 // 2 > 0xffff // 2 and 140000 > 0xffff
    return case([a, b], sub, params=dict(min_baseq=0, min_coverage=1, calling_threshold=1), names=["big"], lengths=[BIG_LEN], seqs=[ref])


def b_two_overhangs(seam_between):
    """SubInfo.flags & 4: contigs of 150 bases, reads 60M at 120 on contig 0 and on contig 1, next to each other in the stream: both run
    past their contig's end.  In one sub-segment the quick round is withdrawn; with a seam between them it stands."""
    refs = [_ref(150, 20 + k) for k in range(3)]
    sub = 128 if seam_between else None
    st = Stream(sub, refs=refs, pos=5)
    st.read(); st.read()
    if seam_between:
        k = st.seam(0)
        i = st.read(pos=120, n=60, seq=refs[0][120:] + "ACGTAC" * 5, size=k * sub - st.off)
    else:
        i = st.read(pos=120, n=60, seq=refs[0][120:] + "ACGTAC" * 5)
    j = st.read(tid=1, pos=120, n=60, seq=refs[1][120:] + "ACGTAC" * 5)
    st.read(tid=2, pos=10)
    assert j == i + 1 and (st.sub_of(i) != st.sub_of(j)) == seam_between
    if seam_between:
        assert st.starts[j] == k * sub
    return case([st], sub, names=["k0", "k1", "k2"], lengths=[150, 150, 150], seqs=refs)


HUGE_LEN = 600200


def b_long_element():
    """maxc_big: a read 30M600000D30M -- its longest pileup element (the deletion's text) does not fit the slot's 19 bits."""
    ref = _ref(HUGE_LEN, 14)
    st = Stream(None, refs=[ref], pos=50)
    st.read(); st.read(cigar="30M600000D30M", pos=100); st.read(pos=120)
    assert 4 + 11 + 600000 >= 0x7ffff
    return case([st], None, names=["huge"], lengths=[HUGE_LEN], seqs=[ref])


# ------------------------------------------------------------------------------------------------ C: what crosses a seam

GAPS = ((0, None), (1, "unm"), (1, "filt"), (1, "long"), (3, "unm"), (3, "filt"), (3, "long"))


def c_bounds(what, sub=128):
    """A sub-segment's first pileup read (a) continues the run and tile group in front of it, (b) opens a new tile of the same contig,
    (c) opens a new contig -- with 0, 1 and 3 sub-segments in between that hold only unmapped records, only filtered ones, or no record
    start at all (the last pileup read in front runs across them)."""
    out = []
    for n_between, gap in GAPS:
        st = Stream(sub, pos=100, tag="%s%d%s" % (what, n_between, (gap or "n")[0]))
        for _ in range(3):
            st.read()
        if gap == "long":
            K = st.off // sub + 1 + n_between
            st.read(size=K * sub - st.off)
        else:
            k1 = st.seam(0)
            st.fill_to(k1 * sub)
            K = k1 + n_between
            st.fill_to(K * sub, gap or "read")
        i = st.read(**{"a": {}, "b": dict(pos=2100), "c": dict(tid=1, pos=50)}[what])
        st.read(); st.read()
        assert st.starts[i] == K * sub and st.kinds[i] == "read"
        between = [st.starts_in(j) for j in range(K - n_between, K)]
        assert all(st.kinds[x] == gap for b in between for x in b) and (gap in (None, "long")) == (not any(between))
        before = [x for x in range(i) if st.kinds[x] == "read"][-1]
        assert st.sub_of(before) < K - n_between
        out.append(st)
    return case(out, sub, many=True)


def c_first_pileup_late(sub=128):
    """The sample's first pileup read is not in its first sub-segment: unmapped records fill the first two, filtered reads the third."""
    st = Stream(sub, pos=100)
    st.fill_to(2 * sub, "unm"); st.fill_to(3 * sub, "filt")
    i = st.read(); st.read(); st.read()
    assert st.starts[i] == 3 * sub and all(k != "read" for k in st.kinds[:i])
    return case([st, plain(sub)], sub)


def c_tile_order(across, sub=256):
    """A read 20D50M at 2040 (its first aligned base lies in the tile at 2048) and behind it 50M at 2045 (the tile in front): the pieces
    need the general tile-order sort.  Both in one sub-segment (the walk sees it), or with a seam between them (msnv_sub_bounds does)."""
    st = Stream(sub, pos=1990)
    st.read(); st.read()
    k = st.seam(0)
    st.fill_to(k * sub)
    if across:
        i = st.read(cigar="20D50M", pos=2040, size=sub)
        j = st.read(n=50, pos=2045)
        assert st.starts[j] == (k + 1) * sub
    else:
        i = st.read(cigar="20D50M", pos=2040)
        j = st.read(n=50, pos=2045)
    st.read(pos=2050); st.read()
    assert (st.sub_of(i) != st.sub_of(j)) == across and j == i + 1
    return case([st, plain(sub)], sub)


def c_order_at_seams(sub=128):
    """Across a seam: two reads at the same position, and a change of contig to a lower position -- neither is out of order."""
    st = Stream(sub, pos=300, step=0)
    st.read()
    k = st.seam(0)
    st.fill_to(k * sub)
    i = st.read()
    assert st.starts[i] == k * sub and st.pos == 300
    st.step = 3
    st.read()
    k = st.seam(0)
    st.fill_to(k * sub)
    j = st.read(tid=1, pos=7)
    assert st.starts[j] == k * sub
    st.read()
    return case([st, plain(sub)], sub)


# ------------------------------------------------------------------------------------------------ D: errors
# Every builder returns (case, which stream fails, which of its records or None, kind); the stream that fails is never the round's first unless said.
# sub = None: no knob is set -- the records are placed against the 6144 bytes of the quick walk (the careful route's own walk then cuts at 4096).
KIND_TEXT = {                         # err_text's phrase (devpack.hip) -> the beginning of pack.cpp's message
    "malformed BAM record": "malformed BAM record at byte",
    "record refers to a contig the header does not have": "record refers to contig",
    "BAM is not coordinate sorted": "BAM is not coordinate sorted",
    "CIGAR and read length disagree": "CIGAR consumes",
}


def _front(sub, tag):
    st = Stream(sub, pos=400, tag=tag)
    st.read(); st.read()
    return st


def d_unsorted_first_of_sub(sub, back):
    """An out-of-order read that is the first mapped record of its sub-segment; the mapped record in front of it starts `back` sub-segments
    earlier, unmapped records between them where they fit."""
    knob, sub = sub, sub or DEFAULT_SUB
    st = _front(sub, "u")
    m = st.seam(44) - 1
    st.fill_to(m * sub + sub - 44)
    p = st.tiny()
    st.fill_to((m + back) * sub + (40 if sub >= 128 else 0), "unm")
    r = st.tiny(pos=st.pos - 100)
    st.read(pos=st.pos + 200)
    assert st.sub_of(p) == m and st.sub_of(r) == m + back and [x for x in st.starts_in(m + back) if st.kinds[x] != "unm"][0] == r
    assert all(st.kinds[x] == "unm" for x in range(p + 1, r))
    return case([plain(sub), st], knob, many=True), 1, r, "BAM is not coordinate sorted"


def d_unsorted_mid_walk(sub):
    """... and one whose predecessor starts in the same sub-segment (the walk itself compares them)."""
    knob, sub = sub, sub or DEFAULT_SUB
    st = _front(sub, "m")
    k = st.seam(0)
    st.fill_to(k * sub)
    p = st.tiny()
    r = st.tiny(pos=st.pos - 100)
    st.read(pos=st.pos + 200)
    assert st.sub_of(p) == st.sub_of(r) == k and r == p + 1
    return case([plain(sub), st], knob, many=True), 1, r, "BAM is not coordinate sorted"


def d_qlen_then_contig(sub):
    """A read whose CIGAR and SEQ disagree, and in a later sub-segment a read of a contig the header does not have: the first in record order is reported."""
    knob, sub = sub, sub or DEFAULT_SUB
    st = _front(sub, "q")
    r = st.read(cigar="30M", seq="ACGT" * 7)
    k = st.seam(0, least=st.sub_of(r) + 2)
    st.fill_to(k * sub)
    t = st.read(tid=len(NAMES) + 2, pos=5)
    assert st.sub_of(t) > st.sub_of(r)
    return case([plain(sub), st], knob, many=True), 1, r, "CIGAR and read length disagree"


def d_unsorted_and_qlen(sub, mid):
    """One read that is out of order AND whose CIGAR and SEQ disagree: pack.cpp looks at the order first."""
    knob, sub = sub, sub or DEFAULT_SUB
    st = _front(sub, "b")
    if mid:
        k = st.seam(0)
        st.fill_to(k * sub)
        p = st.tiny()
        r = st.tiny(pos=st.pos - 100, cigar="2M")
        assert st.sub_of(p) == st.sub_of(r) and r == p + 1
    else:
        k = st.seam(0)
        st.fill_to(k * sub)
        r = st.tiny(pos=st.pos - 100, cigar="2M")
        assert st.starts[r] == k * sub and st.sub_of(r - 1) < k
    st.read(pos=st.pos + 200)
    return case([plain(sub), st], knob, many=True), 1, r, "BAM is not coordinate sorted"


def d_two_streams(sub):
    """Errors in streams 0 and 2 of one round: the first stream's is reported."""
    knob, sub = sub, sub or DEFAULT_SUB
    a = _front(sub, "x"); r = a.read(cigar="30M", seq="ACGT" * 7); a.read()
    c = _front(sub, "z"); c.read(pos=c.pos - 100)
    return case([a, plain(sub), c], knob, many=True), 0, r, "CIGAR and read length disagree"


def d_cut(sub, cut):
    """A stream cut short: by `cut` bytes, or (cut = "header") inside the last record's fixed header.  The chain breaks at the last record's first byte."""
    knob, sub = sub, sub or DEFAULT_SUB
    st = _front(sub, "c")
    st.fill_to(st.seam(-24, least=2) * sub + 24)
    st.read()
    n = len(st.recs[-1]) - 20 if cut == "header" else cut
    c = case([plain(sub), st.bytes(cut=n)], knob, many=True)
    assert 0 < st.off - n - st.starts[-1] < len(st.recs[-1]) and (cut != "header" or st.off - n - st.starts[-1] < 36)
    c.bad_byte = st.starts[-1]
    return c, 1, None, "malformed BAM record"


# ------------------------------------------------------------------------------------------------ E: guesses that fail

ODD_NAMES = {"space": " ", "del": "\x7f", "utf8": "é"}


def e_odd_names(first, sub=128, n_bytes=20000):
    """Every read name begins with a byte hdr_plausible turns down: no sub-segment finds an entry by guessing, each one with a record start
    takes a repair pass of its own."""
    st = Stream(sub, name_first=ODD_NAMES[first], step=2)
    while st.off < n_bytes:
        st.read()
        if len(st.recs) % 5 == 0:
            st.unm(45)
    assert all(not (33 <= r[36] <= 126) for r in st.recs)
    c = case([st], sub)
    c.seams_with_starts = sum(1 for k in range(1, st.n_sub) if st.starts_in(k))
    assert c.seams_with_starts > 100
    return c


def e_pass_limit(sub=64):
    """More than 4096 sub-segments that each need a repair pass: SubWalk::settle gives up, the segment kernel takes the round."""
    st = Stream(sub, name_first=" ", step=2)
    for _ in range(12):
        st.read()
    st.fill_to(st.seam(0, "unm") * sub, "unm")
    k0 = st.off // sub
    while st.n_sub < 4096 + k0 + 8:
        st.unm(64)
    st.unm(64)
    c = case([st], sub)
    c.seams_with_starts = sum(1 for k in range(1, st.n_sub) if st.starts_in(k))
    assert c.seams_with_starts > 4096 + 2
    return c


def e_big_aux(sub):
    """A record with 70 KB of auxiliary bytes (the guess refuses more than 64 KB), records starting in the sub-segments behind it."""
    knob, sub = sub, sub or DEFAULT_SUB
    st = Stream(sub)
    st.read()
    k = st.seam(-9, least=2)
    st.fill_to(k * sub + 9)
    i = st.read(size=70 * 1024 + 200)
    for _ in range(6):
        st.read()
    st.fill_to(st.seam(0, least=st.n_sub + 2) * sub)
    assert st.starts_in(k)[0] == i and st.n_sub - 1 > st.sub_of(i + 1) > k + 8
    return case([st, plain(sub)], knob)


# ------------------------------------------------------------------------------------------------ F: wavefront geometry (64 sub-segments a wavefront)

def f_n_sub(sub=64, counts=(63, 64, 65, 255, 256, 257)):
    """Streams of exactly 63 .. 257 sub-segments; added one by one they are a round each."""
    out = []
    for n in counts:
        st = Stream(sub, tag="n%d" % n, step=1 if n > 200 else 3)
        st.read()
        st.fill_to((n - 1) * sub + 17)
        assert st.n_sub == n
        out.append(st)
    return case(out, sub)


def f_empty_wavefront(sub=64):
    """Sub-segments 64 .. 127 of the round -- the second wavefront's -- hold no record start: its step loop runs zero times."""
    st = Stream(sub)
    st.read()
    st.fill_to(63 * sub + 20)
    i = st.read(size=128 * sub + 7 - st.off)
    st.read(); st.read(); st.read()
    assert st.sub_of(i) == 63 and all(not st.starts_in(k) for k in range(64, 128)) and st.sub_of(i + 1) == 128
    return case([st], sub)


def f_records_per_wavefront(n_rec, sub=128):
    """n_rec records start in the round's first 64 sub-segments: the wavefront writes them 64 a step."""
    lim = 64 * sub
    st = Stream(sub)
    for _ in range(8):
        st.read(size=96)
    u = (lim - st.off) // (n_rec - 8)
    for _ in range(n_rec - 9):
        st.unm(u)
    st.unm(lim + 8 - st.off)
    for _ in range(6):
        st.read()
    assert sum(1 for s in st.starts if s < lim) == n_rec and st.starts[n_rec] == lim + 8
    assert max(len(st.starts_in(k)) for k in range(st.n_sub)) <= cap2(sub)
    return case([st], sub)


def f_many_streams(sub=256, n=70):
    """70 streams of one or two sub-segments in one round, empty ones among them: a wavefront holds sub-segments of many streams."""
    out = []
    for s in range(n):
        if s % 9 == 4:
            out.append(EMPTY)
            continue
        st = Stream(sub, pos=30 + 5 * s, tag="m%d" % s, tid=s % 2)
        for _ in range(1 + s % 4):
            st.read()
        if s % 5 == 0:
            st.unm(40)
        assert 1 <= st.n_sub <= 2
        out.append(st)
    assert sum(1 for x in out if isinstance(x, Stream) and x.n_sub == 2) > 10 and sum(1 for x in out if not isinstance(x, Stream)) > 5
    return case(out, sub, many=True)
