"""A DEFLATE (RFC 1951) WRITER for the tests, and the corpus of hand-assembled streams both decoders of the project are pinned on
(csrc/inflate.cpp on the host, csrc/inflate_k.hip on the device).

A compressor only ever writes a narrow corner of the format, and the two decoders share one design, so neither "streams zlib wrote"
nor "device == host" can see a misreading of the RFC that both share.  This writer takes explicit code lengths, explicit code-length
symbols and explicit tokens, so every construct of the format can be put where a decoder's branches are: the deepest subtables, a
48-bit symbol across the kernel's 256-byte input window, overlapping copies at every small distance, stored blocks behind every bit
offset, and every malformed construct on its own.

The judge is the standard library's zlib (`zlib.decompressobj(-15)`): every case's verdict is COMPUTED from it, never written by hand.
A case is `valid` when zlib ends the stream and returns exactly as many bytes as the member's ISIZE says (which is what htslib asks
of zlib for a BGZF member); for a case meant to be valid the bytes must equal `expand(tokens)` -- that is how the writer itself is
checked -- and a case meant to be malformed must be refused.  `corpus()` asserts both while it generates; nothing is skipped.

Only depends on the standard library.  Deterministic: the same corpus on every call."""
import random
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
WINDOW = 256                     # bytes of compressed input the kernel holds in a register (inflate_k.hip: lane i = dword i)
MEMBER_MAX = 65536 - 26          # the largest payload of a BGZF member: BSIZE is 16 bits, header 18 bytes, trailer 8


# ------------------------------------------------------------------------------------------------------------------ bits and codes
class BitWriter:
    """Bits LSB first, as DEFLATE packs them; Huffman codes go in most significant bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 512:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, c):
        code, nbits = c
        self.put(int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.put(0, -self.bitpos() % 8)

    def raw(self, data):
        assert self.bitpos() % 8 == 0
        self.put(0, 0)
        k = self.n >> 3
        self.out += self.acc.to_bytes(k, "little") if k else b""
        self.acc = 0
        self.n = 0
        self.out += data

    def bytes(self):
        b = BitWriter()
        b.out, b.acc, b.n = bytearray(self.out), self.acc, self.n
        b.align()
        k = b.n >> 3
        return bytes(b.out + (b.acc.to_bytes(k, "little") if k else b""))


def canonical(lengths):
    """(code, bits) of every symbol from its code length (RFC 1951 3.2.2); nothing is checked: over-subscribed and incomplete sets
    get the codes the algorithm gives them (masked to their length)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 = complete, more = over-subscribed, less = incomplete."""
    return sum(1 << (15 - l) for l in lengths if l)


def table_entries(lengths, root):
    """Entries of a two-level decode table for these lengths: 2^root plus, per root prefix that holds longer codes, a subtable of
    2^(longest code under that prefix - root) entries -- how both decoders of the project lay their tables out (for a complete code it
    is what zlib's inflate_table allocates too, whose ENOUGH bounds are the kernel's caps)."""
    deepest = {}
    for c, l in zip(canonical(lengths), lengths):
        if l > root:
            p = c[0] >> (l - root)
            deepest[p] = max(deepest.get(p, 0), l - root)
    return (1 << root) + sum(1 << b for b in deepest.values())


def complete_lengths(n, longest, rnd=None):
    """Sorted code lengths of a COMPLETE code with n symbols whose longest code has `longest` bits: the chain 1, 2, ..., longest,
    longest, then leaves split (seeded choice) until there are n."""
    ls = list(range(1, longest)) + [longest, longest]
    assert len(ls) <= n <= (1 << longest)
    rnd = rnd or random.Random(longest * 1000 + n)
    while len(ls) < n:
        cand = [i for i, l in enumerate(ls) if l < longest]
        i = cand[rnd.randrange(len(cand))]
        ls[i] += 1
        ls.append(ls[i])
    assert kraft(ls) == 32768
    return sorted(ls)


def assign(n_sym, sorted_lengths, short_first=(), rnd=None):
    """Lengths for symbols 0 .. n_sym-1: the symbols of `short_first` take the shortest lengths in that order, the others the rest in
    a seeded order; symbols beyond len(sorted_lengths) get no code."""
    rnd = rnd or random.Random(n_sym * 31 + len(sorted_lengths))
    rest = [s for s in range(n_sym) if s not in set(short_first)]
    rnd.shuffle(rest)
    order = list(short_first) + rest
    lens = [0] * n_sym
    for s, l in zip(order, sorted_lengths):
        lens[s] = l
    return lens


# ------------------------------------------------------------------------------------------------------------------ tokens
# A token is: an int (a literal byte); (length, distance) (a match); (length, distance, "284") (length 258 written as symbol 284 with
# extra bits 31); ("ll", symbol) / ("d", symbol) (a raw literal/length or distance symbol without extra bits: the out-of-range ones).
def length_symbol(length, alt=None):
    if alt == "284":
        assert length == 258
        return 284, 31, 5
    if length == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]


def distance_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


def expand(tokens, start=b""):
    """The bytes a token list stands for, behind `start` (the output of the blocks in front of it)."""
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t[0], str):
            raise ValueError("a raw symbol has no expansion")
        else:
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out), "match reaches in front of the output"
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(start):])


# ------------------------------------------------------------------------------------------------------------------ blocks
def stored_block(bw, data, final, length=None, nlen=None):
    """LEN and NLEN are given separately so that they can disagree; by default they describe `data`."""
    length = len(data) if length is None else length
    nlen = (length ^ 0xffff) if nlen is None else nlen
    bw.put(final, 1); bw.put(0, 2)
    bw.align()
    bw.raw(struct.pack("<HH", length, nlen) + bytes(data))


def put_tokens(bw, tokens, ll_lens, d_lens, eob=True):
    llc, dc = canonical(ll_lens), canonical(d_lens)
    for t in tokens:
        if isinstance(t, int):
            bw.code(llc[t])
        elif t[0] == "ll":
            bw.code(llc[t[1]])
        elif t[0] == "d":
            bw.code(dc[t[1]])
        else:
            s, xv, xb = length_symbol(t[0], t[2] if len(t) > 2 else None)
            bw.code(llc[s]); bw.put(xv, xb)
            s, xv, xb = distance_symbol(t[1])
            bw.code(dc[s]); bw.put(xv, xb)
    if eob:
        bw.code(llc[256])


def fixed_block(bw, tokens, final, eob=True):
    bw.put(final, 1); bw.put(1, 2)
    put_tokens(bw, tokens, FIXED_LL, FIXED_D, eob)


CL_DEFAULT = [4] * 13 + [5] * 6          # a complete code over all 19 code-length symbols


def plain_cl_symbols(lens):
    """The code-length stream without any repeat symbol: (symbol, None) per length."""
    return [(l, None) for l in lens]


def rle_cl_symbols(lens):
    """A greedy run-length coding of the lengths: (symbol, repeat count or None)."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k)); run -= k
            if run >= 3:
                out.append((17, run)); run = 0
            out += [(0, None)] * run
        else:
            out.append((v, None)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k)); run -= k
            out += [(v, None)] * run
        i = j
    return out


def dynamic_header(bw, final, ll_lens, d_lens, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_syms=None):
    """Header of a dynamic block.  ll_lens / d_lens are the lengths the code-length stream carries (len(ll_lens) = HLIT unless `hlit`
    says otherwise; the HLIT / HDIST FIELDS are hlit - 257 and hdist - 1 whatever the lists hold).  cl_lens: the 19 lengths of the
    code-length code (by symbol; the first `hclen` in transmission order are written).  cl_syms: the code-length symbols to write,
    (symbol, count): count is the repeat count of 16 / 17 / 18 and None for a length; default: a greedy run-length coding."""
    hlit = len(ll_lens) if hlit is None else hlit
    hdist = len(d_lens) if hdist is None else hdist
    cl_lens = list(CL_DEFAULT) if cl_lens is None else list(cl_lens)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    if cl_syms is None:
        cl_syms = rle_cl_symbols(list(ll_lens) + list(d_lens))
    bw.put(final, 1); bw.put(2, 2)
    bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl_lens[CL_ORDER[i]], 3)
    clc = canonical(cl_lens)
    for s, k in cl_syms:
        assert clc[s] is not None, "code-length symbol %d has no code" % s
        bw.code(clc[s])
        if s == 16: bw.put(k - 3, 2)
        elif s == 17: bw.put(k - 3, 3)
        elif s == 18: bw.put(k - 11, 7)


def dynamic_block(bw, tokens, final, ll_lens, d_lens, eob=True, **header):
    dynamic_header(bw, final, ll_lens, d_lens, **header)
    put_tokens(bw, tokens, ll_lens, d_lens, eob)


D_DEFAULT = [4, 4] + [5] * 28            # a complete distance code over all 30 symbols


def lengths_for(tokens, n_ll=286, longest=15, d_lens=None, rnd=None):
    """A complete literal/length set over n_ll symbols (longest code `longest` bits) and the default distance set."""
    return assign(n_ll, complete_lengths(n_ll, longest, rnd), rnd=rnd), list(D_DEFAULT if d_lens is None else d_lens)


# ------------------------------------------------------------------------------------------------------------------ BGZF
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf(members, eof=True, align=None):
    """A BGZF file from (raw deflate payload, intended uncompressed bytes) pairs, plus the EOF member.  The trailer's CRC-32 and ISIZE
    are always those of the INTENDED bytes.  align: per member None or 0..3 -- a second gzip extra subfield ("PD", zeros) is put behind
    the BC one so that the payload starts at that file offset mod 4 (the device keeps file offsets: the kernel's `a0`)."""
    out = bytearray()
    for k, (comp, data) in enumerate(members):
        pad = b""
        if align is not None and align[k] is not None:
            n = (align[k] - (len(out) + 18 + 4)) % 4
            pad = b"PD" + struct.pack("<H", n) + bytes(n)
        bsize = 18 + len(pad) + len(comp) + 8
        assert bsize <= 65536, "a BGZF member holds at most 65536 bytes"
        out += bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", 6 + len(pad)) + b"BC\x02\x00" + struct.pack("<H", bsize - 1) + pad
        out += comp + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))
    if eof:
        out += EOF_MEMBER
    return bytes(out)


def payload_offsets(file_bytes):
    """File offset of every member's deflate payload (what the device's InfBlock::in_off is, for the first file of a batch)."""
    offs, off = [], 0
    while off < len(file_bytes):
        xlen = file_bytes[off + 10] | file_bytes[off + 11] << 8
        offs.append(off + 12 + xlen)
        off += (file_bytes[off + 16] | file_bytes[off + 17] << 8) + 1
    return offs


# ------------------------------------------------------------------------------------------------------------------ the judge
def judge(stream, isize):
    """zlib's verdict on a raw stream that claims `isize` bytes: the bytes, or None (an error, an unfinished stream, another size)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream) + d.flush()
    except zlib.error:
        return None
    return out if d.eof and len(out) == isize else None


class Case:
    __slots__ = ("name", "family", "stream", "intended", "valid", "align")

    def __init__(self, name, family, stream, intended, valid, align=None):
        self.name, self.family, self.stream, self.intended, self.valid, self.align = name, family, bytes(stream), bytes(intended), valid, align
        assert len(self.stream) <= MEMBER_MAX, (name, len(self.stream))
        got = judge(self.stream, len(self.intended))
        if valid:
            assert got == self.intended, "%s: the writer and zlib disagree on a stream meant to be valid" % name
        else:
            assert got is None, "%s: zlib accepts a stream meant to be malformed" % name

    def __repr__(self):
        return "<%s %s: %d -> %d bytes>" % ("valid" if self.valid else "malformed", self.name, len(self.stream), len(self.intended))


def pattern(n, seed=0):
    """n bytes without short periods (so that a copy from the wrong place is a wrong byte)."""
    r = random.Random(seed * 7919 + n)
    return [r.randrange(256) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------ valid families
# The sets that need the most table entries come from a seeded hill-climb over complete codes (maximising table_entries): a 286-symbol
# code under a 9-bit root (the kernel; zlib's bound is 852) and under an 11-bit root (the host decoder), a 30-symbol code under a 6-bit
# (592) and an 8-bit root.  What each climb reached is kept here, by (table, seed), for the tests to compare with the decoders' caps.
MAX_TABLE_HISTS = {}        # filled by gen_code_shapes()


def _climb(n, root, seed, steps=4000):
    """Hill-climb on sorted complete length lists of n symbols: move = split one leaf and merge two others of equal length (keeps the
    symbol count and completeness)."""
    rnd = random.Random(seed)
    ls = complete_lengths(n, 15, rnd)
    best = table_entries(ls, root)
    for _ in range(steps):
        cand = list(ls)
        i = rnd.randrange(n)
        if cand[i] >= 15:
            continue
        pairs = [l for l in set(cand) if l > 1 and cand.count(l) >= (3 if l == cand[i] else 2)]
        if not pairs:
            continue
        m = pairs[rnd.randrange(len(pairs))]
        cand[i] += 1
        cand.append(cand[i])
        cand.remove(m); cand.remove(m); cand.append(m - 1)
        cand.sort()
        if kraft(cand) != 32768 or len(cand) != n:
            continue
        t = table_entries(cand, root)
        if t >= best:
            ls, best = cand, t
    return ls, best


def gen_code_shapes():
    body = pattern(300, 1)
    toks = list(range(256)) + body + [(3, 1), (10, 17), (258, 300), (131, 64), (67, 5)]
    for longest in range(9, 16):
        ll, d = lengths_for(toks, 286, longest)
        bw = BitWriter(); dynamic_block(bw, toks, 1, ll, d)
        yield Case("ll_longest_%d" % longest, "code_shapes", bw.bytes(), expand(toks), True)
    for longest in range(7, 16):
        ll, _ = lengths_for(toks, 286, 12)
        d = assign(30, complete_lengths(30, longest))
        t2 = toks + [(5, DIST_BASE[s]) for s in range(17)] + [(4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1) for s in range(17)]
        bw = BitWriter(); dynamic_block(bw, t2, 1, ll, d)
        yield Case("d_longest_%d" % longest, "code_shapes", bw.bytes(), expand(t2), True)
    # subtables as large as they can be: under a 9-bit root a prefix whose longest code has 15 bits needs 64 entries, under the
    # distance code's 6-bit root 512; the chain 1, 2, ..., 15, 15 puts the long codes under one prefix, splitting its short leaves
    # spreads them over many
    for name, n, rnd_seed in (("ll_deep_subtables", 286, 3), ("ll_deep_subtables_b", 286, 4)):
        ll = assign(286, complete_lengths(286, 15, random.Random(rnd_seed)), rnd=random.Random(rnd_seed))
        d = assign(30, complete_lengths(30, 15, random.Random(rnd_seed)), rnd=random.Random(rnd_seed))
        t2 = toks + [(4, DIST_BASE[s]) for s in range(17)]
        bw = BitWriter(); dynamic_block(bw, t2, 1, ll, d)
        yield Case(name, "code_shapes", bw.bytes(), expand(t2), True)
    chain = list(range(1, 15)) + [15, 15]                      # 16 symbols: ONE subtable of the largest size at either root
    ll = [0] * 286
    for s, l in zip([97, 256, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 284, 285, 257], chain):
        ll[s] = l
    d = [0] * 30
    for s, l in zip([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 29, 28], chain):
        d[s] = l
    t3 = [97 + (i * 5) % 12 for i in range(300)] + [(258, 1), (3, 2), (258, 100, "284"), (258, 3)] * 40 + [(258, 65), (258, 16385), (258, 24577), (227, 24578)]
    bw = BitWriter(); dynamic_block(bw, t3, 1, ll, d)
    yield Case("chain_1_to_15_both", "code_shapes", bw.bytes(), expand(t3), True)
    # HLIT = 257 (no length symbol) with HDIST = 1 and a zero length: a block of literals only
    ll = assign(257, complete_lengths(257, 11))
    t4 = list(range(256)) + body
    bw = BitWriter(); dynamic_block(bw, t4, 1, ll, [0])
    yield Case("hlit257_hdist1_no_distance_code", "code_shapes", bw.bytes(), expand(t4), True)
    # HDIST = 1 with one code of one bit (the incomplete set zlib allows): every match is at distance 1
    ll, _ = lengths_for(toks, 286, 10)
    t5 = body[:70] + [(258, 1), 7, (3, 1), (64, 1), (65, 1), 9, 9, (129, 1)]
    bw = BitWriter(); dynamic_block(bw, t5, 1, ll, [1])
    yield Case("hdist1_one_code_of_one_bit", "code_shapes", bw.bytes(), expand(t5), True)
    ll, d = lengths_for(toks, 286, 13)                         # HLIT = 286, HDIST = 30
    t6 = toks + [(4, DIST_BASE[s]) for s in range(17)]
    bw = BitWriter(); dynamic_block(bw, t6, 1, ll, d, cl_syms=plain_cl_symbols(ll + d))
    yield Case("hlit286_hdist30_no_repeats", "code_shapes", bw.bytes(), expand(t6), True)
    # HCLEN: 19 (a code-length code over all 19 symbols, above) and the smallest a valid block can have.  HCLEN = 4 only gives lengths
    # to 16, 17, 18 and 0, so no symbol can get a code at all: it is among the malformed cases; HCLEN = 5 adds length 8 -- exactly
    # 256 symbols of 8 bits, the end-of-block code among them
    ll = [8] * 255 + [0, 8]
    cl = [0] * 19; cl[8] = 1; cl[0] = 1
    t7 = [i for i in body if i != 255]
    bw = BitWriter(); dynamic_block(bw, t7, 1, ll, [0], cl_lens=cl, cl_syms=plain_cl_symbols(ll + [0]))
    yield Case("hclen5_the_smallest_valid", "code_shapes", bw.bytes(), expand(t7), True)
    cl = [0] * 19; cl[8] = 2; cl[0] = 2; cl[16] = 2; cl[18] = 2
    bw = BitWriter(); dynamic_block(bw, t7, 1, ll, [0], cl_lens=cl, hclen=19)
    yield Case("hclen19_with_four_codes", "code_shapes", bw.bytes(), expand(t7), True)
    # the sets that need the most table entries
    for key, (n, root) in (("ll_root9", (286, 9)), ("ll_root11", (286, 11)), ("d_root6", (30, 6)), ("d_root8", (30, 8))):
        for seed in (1, 2, 3):
            ls, size = _climb(n, root, seed * 100 + root)
            MAX_TABLE_HISTS[(key, seed)] = size
            assert size <= {9: 852, 11: 2048 + 915, 6: 592, 8: 256 + 480}[root], (key, size)
            if n == 286:
                ll = assign(286, ls, rnd=random.Random(seed)); d = list(D_DEFAULT); tt = toks
            else:
                ll, _ = lengths_for(toks, 286, 9); d = assign(30, ls, rnd=random.Random(seed))
                tt = toks + [(4, DIST_BASE[s]) for s in range(17)]
            bw = BitWriter(); dynamic_block(bw, tt, 1, ll, d)
            yield Case("max_table_%s_%d_entries_%d" % (key, seed, size), "max_tables", bw.bytes(), expand(tt), True)


def gen_code_length_stream():
    body = pattern(200, 2)
    toks = body + [(20, 7), (258, 30)]
    # 16 repeating across the literal -> distance boundary: the last literal/length lengths and the first distance lengths are equal
    # (symbols 283 .. 285 and distance symbols 0 .. 3 all have 9 bits; 1/2 + ... + 1/128 + 4/512 is a complete distance set)
    ll_sorted = complete_lengths(286, 9, random.Random(6))
    assert ll_sorted[-3:] == [9, 9, 9]
    ll = assign(286, ll_sorted, short_first=[s for s in range(283) if s % 2], rnd=random.Random(7))
    ll[283:] = [9, 9, 9]
    assert kraft(ll) == 32768
    d = [9, 9, 9, 9, 1, 2, 3, 4, 5, 6, 7]
    syms = rle_cl_symbols(ll[:283]) + [(9, None), (16, 6)] + plain_cl_symbols(d[4:])      # 283 is written; 16 x 6 is 284, 285 and distance 0 .. 3
    bw = BitWriter(); dynamic_block(bw, toks, 1, ll, d, cl_syms=syms)
    yield Case("repeat16_across_the_table_boundary", "code_length_stream", bw.bytes(), expand(toks), True)
    # 18 with 138, 17 with 3 and with 10: a literal/length set with long stretches of unused symbols
    ll = [0] * 286
    used = [0, 1, 2] + [141, 142] + [146] + [157] + [256] + list(range(268, 286))      # gaps of 138 (3..140), 3 (143..145), 10 (147..156), 98, 11
    for s, l in zip(used, complete_lengths(len(used), 7, random.Random(8))):
        ll[s] = l
    syms = plain_cl_symbols(ll[:3]) + [(18, 138)] + plain_cl_symbols(ll[141:143]) + [(17, 3)] + plain_cl_symbols(ll[146:147]) + [(17, 10)] + \
        plain_cl_symbols(ll[157:158]) + [(18, 98)] + plain_cl_symbols(ll[256:257]) + [(18, 11)] + plain_cl_symbols(ll[268:]) + rle_cl_symbols(D_DEFAULT)
    t2 = [0, 1, 2, 141, 142, 146, 157] * 9 + [(258, 5), (17, 63), (35, 2)]
    bw = BitWriter(); dynamic_block(bw, t2, 1, ll, D_DEFAULT, cl_syms=syms)
    yield Case("repeat18_138_repeat17_3_and_10", "code_length_stream", bw.bytes(), expand(t2), True)
    # a run that ends exactly at HLIT + HDIST: the last symbol is a repeat (18 x 29 zeros: distance symbols 1 .. 29; 16 x 6; 17 x 7)
    ll, _ = lengths_for(toks, 286, 9)
    t3 = body + [(258, 1), (4, 1)]
    for name, d, tail in (("zeros_by_18", [1] + [0] * 29, [(1, None), (18, 29)]), ("zeros_by_17", [1] + [0] * 7, [(1, None), (17, 7)]),
                          ("copies_by_16", [3] * 7 + [0] + [3], [(3, None), (16, 6), (0, None), (3, None)]), ("copies_by_16_last", [1, 2] + [5] * 8, [(1, None), (2, None), (5, None), (5, None), (16, 6)])):
        tt = t3 if d[0] == 1 else body + [(258, 1), (4, 2), (9, 3), (9, 4)]
        bw = BitWriter(); dynamic_block(bw, tt, 1, ll, d, cl_syms=rle_cl_symbols(ll) + tail)
        yield Case("run_ends_at_hlit_plus_hdist_%s" % name, "code_length_stream", bw.bytes(), expand(tt), True)


def gen_every_symbol():
    pre = pattern(400, 3)
    # every length symbol at its lowest and highest extra-bits value; fixed codes and a dynamic set with long codes for the length symbols
    toks = list(pre)
    for s in range(29):
        for v in sorted({0, (1 << LEN_EXTRA[s]) - 1}):
            toks += [(LEN_BASE[s] + v, 3 + s * 11), pre[s]]
    toks += [(258, 300, "284"), 1, (258, 300), 2, (258, 1, "284"), (258, 2)]
    bw = BitWriter(); fixed_block(bw, toks, 1)
    yield Case("every_length_symbol_fixed", "every_symbol", bw.bytes(), expand(toks), True)
    ll = assign(286, complete_lengths(286, 15, random.Random(9)), short_first=list(range(0, 256, 3)))      # literals short, length symbols long
    bw = BitWriter(); dynamic_block(bw, toks, 1, ll, D_DEFAULT)
    yield Case("every_length_symbol_dynamic", "every_symbol", bw.bytes(), expand(toks), True)
    # every distance symbol likewise, distance 32768 included: the output in front of it is grown by long matches
    toks = list(pre) + [(258, 400)] * 127                      # 400 + 32766 bytes
    toks += [5, 6]                                             # 33168
    for s in range(30):
        for v in sorted({0, (1 << DIST_EXTRA[s]) - 1}):
            toks += [(3 + s, DIST_BASE[s] + v), pre[s + 50]]
    assert (3 + 29, 32768) in toks
    bw = BitWriter(); fixed_block(bw, toks, 1)
    yield Case("every_distance_symbol_fixed", "every_symbol", bw.bytes(), expand(toks), True)
    d = assign(30, complete_lengths(30, 15, random.Random(10)), short_first=[15])
    ll, _ = lengths_for(toks, 286, 12)
    bw = BitWriter(); dynamic_block(bw, toks, 1, ll, d)
    yield Case("every_distance_symbol_dynamic", "every_symbol", bw.bytes(), expand(toks), True)


OVERLAP_LENGTHS = [3, 4, 63, 64, 65, 127, 128, 129, 257, 258]


def gen_overlap():
    residues = set()
    for dist in range(1, 131):
        toks = pattern(130 + (dist * 37) % 64, dist)
        n = len(toks)
        for k, length in enumerate(OVERLAP_LENGTHS[dist % 10:] + OVERLAP_LENGTHS[:dist % 10]):
            residues.add(n % 64)
            toks.append((length, dist)); n += length
            if k % 3 != 2:
                toks.append((dist * 3 + k) % 256); n += 1
        toks.append((OVERLAP_LENGTHS[dist % 10], dist))                       # the match ends on the block's last byte: EOB follows it
        bw = BitWriter()
        if dist % 2:
            fixed_block(bw, toks, 1)
        else:
            ll, d = lengths_for(toks, 286, 9 + dist % 7)
            dynamic_block(bw, toks, 1, ll, d)
        yield Case("distance_%d" % dist, "overlap", bw.bytes(), expand(toks), True)
    # all residues mod 64 of the match's output offset, at the distances below one step of the kernel's copy
    for r in range(64):
        toks = pattern(64 + r, 500 + r)
        for dist in (1, 2, 3, 5, 31, 32, 33, 63):
            residues.add(len(expand(toks)) % 64)
            toks += [(128, dist)]
        bw = BitWriter(); fixed_block(bw, toks, 1)
        yield Case("offset_residue_%d" % r, "overlap", bw.bytes(), expand(toks), True)
    assert residues == set(range(64))
    # output of exactly 65536 bytes, the last match ending on the last byte
    toks = pattern(256, 77)
    n = 256
    k = 0
    while n + 258 <= 65536 - 3:
        toks.append((258, [1, 7, 64, 200, 255, 256][k % 6])); n += 258; k += 1
    while 65536 - n > 258 + 3:
        toks.append(k % 256); n += 1
    rest = 65536 - n
    if rest > 258:
        toks.append((rest - 258 if rest - 258 >= 3 else 3, 9)); n += toks[-1][0]
        rest = 65536 - n
    toks.append((rest, 61))
    out = expand(toks)
    assert len(out) == 65536
    bw = BitWriter(); fixed_block(bw, toks, 1)
    yield Case("output_of_65536_bytes", "overlap", bw.bytes(), out, True)


# The widest symbol: a 15-bit length code + 5 extra bits + a 15-bit distance code + 13 extra bits = 48 bits, all the kernel's refill(48)
# promises.  Literal/length lengths: 'a' and symbol 285 two bits, 'b' and end-of-block three, then the chain 3 .. 15, 15 with symbol
# 284 on 15 bits; distance lengths: symbol 0 one bit, then the chain 2 .. 15, 15 with symbols 28 and 29 on 15 bits.  (258, 1) costs three
# bits, so a few hundred bits grow the output past 16385 bytes; 'a' (2 bits) and 'b' (3 bits) then put the wide symbol at any bit.
def _wide_sets():
    ll = [0] * 286
    ll[97] = 2; ll[285] = 2; ll[98] = 3; ll[256] = 3
    for s, l in zip([99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 284, 283], list(range(3, 15)) + [15, 15]):
        ll[s] = l
    d = [0] * 30
    for s, l in zip([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 29, 28], [1] + list(range(2, 15)) + [15, 15]):
        d[s] = l
    assert kraft(ll) == 32768 and kraft(d) == 32768
    return ll, d


def wide_symbol_stream(target_bit):
    """A stream whose wide symbol starts `target_bit` bits into the payload.  Returns (stream, tokens)."""
    ll, d = _wide_sets()
    bw = BitWriter()
    dynamic_header(bw, 1, ll, d)
    toks = [97, 98, 99, 100] + [(258, 1)] * 100                    # 4 + 25800 bytes for 2 + 3 + 3 + 4 + 100 * 3 bits
    put_tokens(bw, toks, ll, d, eob=False)
    fill = target_bit - bw.bitpos()
    assert fill >= 2, (target_bit, bw.bitpos())
    lits = [98] * (fill % 2) + [97] * ((fill - 3 * (fill % 2)) // 2)
    assert 2 * lits.count(97) + 3 * lits.count(98) == fill
    tail = [(258, 16385 + 8191, "284"), 99, (258, 24577, "284"), 100]      # symbol 284 + 31, distance symbol 28 + 8191: 15 + 5 + 15 + 13 bits
    put_tokens(bw, lits, ll, d, eob=False)
    assert bw.bitpos() == target_bit
    put_tokens(bw, tail, ll, d, eob=True)
    return bw.bytes(), toks + lits + tail


def gen_window():
    for a0 in range(4):
        for seam in (1, 3):
            seam_bit = 8 * (WINDOW * seam - a0)                    # the windows start at the aligned address in front of the payload
            for off in range(-48, 9):
                stream, toks = wide_symbol_stream(seam_bit + off)
                yield Case("wide_symbol_a0_%d_seam_%d_at_%+d" % (a0, seam, off), "window", stream, expand(toks), True, align=a0)


def gen_literal_batching():
    for n in (63, 64, 65, 129):
        lits = pattern(n, n)
        for behind in ("match", "eob", "stored"):
            for dyn in (0, 1):
                bw = BitWriter()
                toks = lits + ([(70, n - 1), 5] if behind == "match" else [])
                if dyn:
                    ll, d = lengths_for(toks, 286, 11)
                    dynamic_block(bw, toks, behind != "stored", ll, d)
                else:
                    fixed_block(bw, toks, behind != "stored")
                out = expand(toks)
                if behind == "stored":
                    more = bytes(pattern(77, n + 1))
                    stored_block(bw, more, 1)
                    out += more
                yield Case("%d_literals_then_%s_%s" % (n, behind, "dynamic" if dyn else "fixed"), "literal_batching", bw.bytes(), out, True)


def gen_stored():
    for n in (0, 1, 255, 256, 257, MEMBER_MAX - 5):
        data = bytes(pattern(n, n))
        bw = BitWriter(); stored_block(bw, data, 1)
        yield Case("stored_len_%d" % n, "stored", bw.bytes(), data, True)
    # behind a Huffman block that ends at each of the 8 bit offsets (fixed codes: a literal below 144 is 8 bits, above 9, EOB 7)
    seen = set()
    for k in range(8):
        toks = [200] * k + [1, 2, 3]
        bw = BitWriter(); fixed_block(bw, toks, 0)
        seen.add((bw.bitpos() + 3) % 8)                            # where the stored block's 3 header bits end
        data = bytes(pattern(300, k))
        stored_block(bw, data, 1)
        yield Case("stored_behind_huffman_ending_at_bit_%d" % ((3 + 9 * k + 24 + 7) % 8), "stored", bw.bytes(), expand(toks) + data, True)
    assert seen == set(range(8))
    # the LEN / NLEN words around a window seam: the Huffman block in front ends so that LEN starts from 12 bytes before to 4 bytes
    # behind the seam, for every start alignment; its end-of-block code is 1, 2 or 7 bits, so that the bit buffer the stored block
    # meets holds from no byte to several bytes behind NLEN -- those go back to the input, also across the seam (resync backwards)
    for a0 in range(4):
        for eob_bits in (1, 2, 7):
            for at in range(-12, 5):
                len_byte = WINDOW - a0 + at
                bw = BitWriter()
                if eob_bits == 7:
                    n_lit = len_byte - 2                           # 3 header bits + 8 n + 7 + 3 header bits -> ends inside byte n + 1
                    toks = [(i * 7) % 144 for i in range(n_lit)]
                    fixed_block(bw, toks, 0)
                else:
                    ll = [0] * 257
                    if eob_bits == 1:
                        ll[256] = 1; ll[65] = 2; ll[66] = 3; ll[67] = 3
                    else:
                        ll[256] = 2; ll[65] = 1; ll[66] = 3; ll[67] = 3
                    dynamic_header(bw, 0, ll, [0])
                    bits_left = 8 * len_byte - bw.bitpos() - eob_bits - 3
                    assert bits_left > 16
                    toks = [66, 67] * 2                            # 12 bits, then 'A's up to the last few bits
                    w = 2 if eob_bits == 1 else 1
                    room = bits_left - 12                          # (a last odd bit may stay free: the stored header pads to the byte)
                    toks += [65] * (room // w)
                    put_tokens(bw, toks, ll, [0])
                assert (bw.bitpos() + 3 + 7) // 8 == len_byte, (bw.bitpos(), len_byte)      # LEN is the first whole byte behind the 3 header bits
                data = bytes(pattern(40, at + 20))
                stored_block(bw, data, 0)
                t2 = [9, 8, (30, 20), 7]
                fixed_block(bw, t2, 1)
                head = expand(toks) + data
                yield Case("len_word_a0_%d_eob_%d_bits_at_%+d" % (a0, eob_bits, at), "stored_seam", bw.bytes(), head + expand(t2, head), True, align=a0)
    # stored blocks long enough to skip more than one window, Huffman blocks between them
    for n in (255, 256, 257, 511, 513, 700, 1024, 5000):
        bw = BitWriter(); out = b""
        for k in range(3):
            data = bytes(pattern(n + k, n + k)); stored_block(bw, data, 0); out += data
            t = [1, 2, 3, (50, n // 2 + 1), 4]
            fixed_block(bw, t, 0); out += expand(t, out)
        stored_block(bw, b"", 1)
        yield Case("stored_skips_%d_bytes_then_huffman" % n, "stored", bw.bytes(), out, True)
    # stored -> Huffman -> stored, the Huffman block's matches reaching back into the stored bytes (and through them)
    first = bytes(pattern(500, 41))
    bw = BitWriter(); stored_block(bw, first, 0)
    t = [(258, 500), 1, (100, 259), (40, 1), (258, 858)]
    ll, d = lengths_for(t, 286, 14)
    dynamic_block(bw, t, 0, ll, d)
    out = first + expand(t, first)
    last = bytes(pattern(300, 42)); stored_block(bw, last, 1)
    yield Case("stored_huffman_stored_with_matches_into_the_stored_bytes", "stored", bw.bytes(), out + last, True)


def gen_several_blocks():
    bw = BitWriter(); out = b""
    ll, d = lengths_for([], 286, 9)
    for k in range(5):
        fixed_block(bw, [], 0)
        dynamic_block(bw, [], 0, ll, d)
    t = pattern(100, 50) + [(20, 100)]
    fixed_block(bw, t, 0); out = expand(t)
    dynamic_block(bw, [], 0, ll, d); fixed_block(bw, [], 1)
    yield Case("empty_fixed_and_dynamic_blocks_not_final", "several_blocks", bw.bytes(), out, True)
    bw = BitWriter(); out = b""
    rnd = random.Random(60)
    for k in range(90):
        kind = k % 3
        if kind == 0:
            data = bytes(pattern(rnd.randrange(4), k)); stored_block(bw, data, 0); out += data
        else:
            t = pattern(1 + rnd.randrange(3), k) + [(3 + rnd.randrange(6), 1 + rnd.randrange(min(len(out) + 1, 40)))]
            if kind == 1:
                fixed_block(bw, t, 0)
            else:
                l2 = assign(286, complete_lengths(286, 9 + k % 7, random.Random(k)), rnd=random.Random(k))
                dynamic_block(bw, t, 0, l2, D_DEFAULT)
            out += expand(t, out)
    fixed_block(bw, [0], 1); out += b"\0"
    yield Case("ninety_tiny_blocks", "several_blocks", bw.bytes(), out, True)
    # an empty member: a final block without output (ISIZE 0) in each of the three forms, and the incomplete sets zlib allows
    for name, make in (("stored", lambda b: stored_block(b, b"", 1)), ("fixed", lambda b: fixed_block(b, [], 1)), ("dynamic", lambda b: dynamic_block(b, [], 1, ll, d))):
        bw = BitWriter(); make(bw)
        yield Case("empty_member_%s" % name, "several_blocks", bw.bytes(), b"", True)


VALID_GENERATORS = [gen_code_shapes, gen_code_length_stream, gen_every_symbol, gen_overlap, gen_window, gen_literal_batching, gen_stored,
                    gen_several_blocks]


# ------------------------------------------------------------------------------------------------------------------ malformed families
def gen_malformed():
    body = pattern(120, 70)
    good = body + [(30, 17), 1, 2, 3]
    ll, d = lengths_for(good, 286, 10)
    want = expand(good)

    def case(name, bw_or_bytes, intended, valid=False, family="malformed"):
        s = bw_or_bytes if isinstance(bw_or_bytes, (bytes, bytearray)) else bw_or_bytes.bytes()
        return Case(name, family, s, intended, valid)

    bw = BitWriter(); fixed_block(bw, body, 0); bw.put(1, 1); bw.put(3, 2); bw.put(0, 13)
    yield case("block_type_3", bw, bytes(body))
    bw = BitWriter(); stored_block(bw, bytes(body), 1, nlen=(len(body) ^ 0xffff) ^ 0x0100)
    yield case("stored_len_nlen_mismatch", bw, bytes(body))
    for hlit in (287, 288):
        bw = BitWriter(); dynamic_block(bw, good, 1, ll + [0] * (hlit - 286), d)
        yield case("hlit_%d" % hlit, bw, want)
    for hdist in (31, 32):
        bw = BitWriter(); dynamic_block(bw, good, 1, ll, d + [0] * (hdist - 30))
        yield case("hdist_%d" % hdist, bw, want)
    # HCLEN = 4: only 16, 17, 18 and 0 can have a code, so every length is 0 and there is no end-of-block code
    cl = [0] * 19; cl[0] = 1; cl[18] = 1
    bw = BitWriter(); dynamic_header(bw, 1, [0] * 257, [0], cl_lens=cl, hclen=4, cl_syms=[(18, 138), (18, 120)])
    yield case("hclen_4_cannot_code_any_symbol", bw, b"")
    # the three sets, each over-subscribed / incomplete / incomplete in the one form zlib's table builder allows
    cl = list(CL_DEFAULT); cl[3] = 3                               # 13 x 4 bits + 6 x 5 bits is complete: one code shorter over-subscribes
    bw = BitWriter(); dynamic_block(bw, good, 1, ll, d, cl_lens=cl)
    yield case("code_length_set_over_subscribed", bw, want)
    cl = list(CL_DEFAULT); cl[3] = 5
    bw = BitWriter(); dynamic_block(bw, good, 1, ll, d, cl_lens=cl)
    yield case("code_length_set_incomplete", bw, want)
    cl = [0] * 19; cl[18] = 1                                      # one code of one bit: allowed for distances, not for this set
    bw = BitWriter(); dynamic_header(bw, 1, [0] * 257, [0], cl_lens=cl, cl_syms=[(18, 138), (18, 120)])
    yield case("code_length_set_one_code_of_one_bit", bw, b"")
    bw = BitWriter(); dynamic_header(bw, 1, [0] * 257, [0], cl_lens=[0] * 19, hclen=19, cl_syms=[]); bw.put(0, 64)
    yield case("code_length_set_without_any_code", bw, b"")
    over = list(ll); i = max(range(256), key=lambda s: ll[s]); over[i] -= 1
    bw = BitWriter(); dynamic_block(bw, good, 1, over, d)
    yield case("literal_length_set_over_subscribed", bw, want)
    # (the issue's probe) 'a' one bit, end-of-block two bits: every code the stream uses exists, a quarter of the code space is a hole
    l2 = [0] * 257; l2[97] = 1; l2[256] = 2
    bw = BitWriter(); dynamic_block(bw, [97] * 50, 1, l2, [0])
    yield case("literal_length_set_incomplete", bw, b"a" * 50)
    under = list(ll); under[i] += 1
    bw = BitWriter(); dynamic_block(bw, good, 1, under, d)
    yield case("literal_length_set_incomplete_by_one_long_code", bw, want)
    # the form zlib allows: a single code of one bit -- which can only be the end-of-block code: an empty block (in front of a real one)
    l3 = [0] * 257; l3[256] = 1
    bw = BitWriter(); dynamic_block(bw, [], 0, l3, [0]); fixed_block(bw, good, 1)
    yield case("literal_length_set_of_one_code_of_one_bit", bw, want, valid=True)
    bw = BitWriter(); dynamic_block(bw, body + [(30, 1), (30, 2)], 1, ll, [1, 1, 1])
    yield case("distance_set_over_subscribed", bw, expand(body + [(30, 1), (30, 2)]))
    bw = BitWriter(); dynamic_block(bw, body + [(30, 1), (30, 2)], 1, ll, [2, 2])
    yield case("distance_set_incomplete", bw, expand(body + [(30, 1), (30, 2)]))
    bw = BitWriter(); dynamic_block(bw, body + [(30, 2)], 1, ll, [0, 2])
    yield case("distance_set_one_code_of_two_bits", bw, expand(body + [(30, 2)]))
    bw = BitWriter(); dynamic_block(bw, body + [(258, 1)], 1, ll, [1])
    yield case("distance_set_of_one_code_of_one_bit", bw, expand(body + [(258, 1)]), valid=True)
    bw = BitWriter(); dynamic_block(bw, body + [(258, 2)], 1, ll, [0, 1])
    yield case("distance_set_of_one_code_of_one_bit_second_symbol", bw, expand(body + [(258, 2)]), valid=True)
    bw = BitWriter(); dynamic_header(bw, 1, ll, [0, 0, 0], cl_syms=rle_cl_symbols(ll) + [(0, None)] * 3)
    put_tokens(bw, body + [("ll", 257 + 5)], ll, [0, 0, 0], eob=False); bw.put(0, 6); put_tokens(bw, [], ll, [0, 0, 0])
    yield case("distance_set_without_any_code_and_a_match", bw, bytes(body) + b"x" * 8)
    # the used code of a one-code distance set is '0': '1' is a hole
    bw = BitWriter(); dynamic_header(bw, 1, ll, [1]); put_tokens(bw, body + [("ll", 257)], ll, [1], eob=False); bw.put(1, 1); put_tokens(bw, [], ll, [1])
    yield case("distance_code_in_the_hole_of_a_one_code_set", bw, bytes(body) + b"xxx")
    # the code-length stream
    bw = BitWriter(); dynamic_block(bw, good, 1, ll, d, cl_syms=[(16, 3)] + rle_cl_symbols(ll[3:] + d))
    yield case("repeat_16_as_the_first_code_length_symbol", bw, want)
    bw = BitWriter(); dynamic_block(bw, good, 1, ll, d, cl_syms=rle_cl_symbols(ll + d[:-1]) + [(16, 3)])
    yield case("repeat_16_overruns_hlit_plus_hdist", bw, want)
    bw = BitWriter(); dynamic_block(bw, good, 1, ll, [4, 4] + [5] * 20, hdist=30, cl_syms=rle_cl_symbols(ll + [4, 4] + [5] * 20) + [(18, 11)])
    yield case("repeat_18_overruns_hlit_plus_hdist", bw, want)
    noeob = list(ll); noeob[256] = 0
    bw = BitWriter(); dynamic_header(bw, 1, noeob, d); put_tokens(bw, good, noeob, d, eob=False); bw.put(0, 40)
    yield case("no_end_of_block_code", bw, want)
    # symbols the fixed codes have room for and the format does not define
    for s in (286, 287):
        bw = BitWriter(); fixed_block(bw, body + [("ll", s), ("d", 0)], 1)
        yield case("fixed_literal_length_symbol_%d" % s, bw, bytes(body) + b"xxx")
    for s in (30, 31):
        bw = BitWriter(); fixed_block(bw, body + [("ll", 257), ("d", s)], 1)
        yield case("fixed_distance_symbol_%d" % s, bw, bytes(body) + b"xxx")
    # a distance that reaches in front of the output
    bw = BitWriter(); fixed_block(bw, [("ll", 257), ("d", 0), 1, 2], 1)
    yield case("distance_at_output_position_0", bw, b"xxx\1\2")
    for dyn in (0, 1):
        t = body[:50] + [("ll", 257 + 2)]
        bw = BitWriter()
        if dyn:
            dynamic_header(bw, 1, ll, d); put_tokens(bw, t, ll, d, eob=False)
            s, xv, xb = distance_symbol(51); bw.code(canonical(d)[s]); bw.put(xv, xb); put_tokens(bw, [], ll, d)
        else:
            bw.put(1, 1); bw.put(1, 2); put_tokens(bw, t, FIXED_LL, FIXED_D, eob=False)
            s, xv, xb = distance_symbol(51); bw.code(canonical(FIXED_D)[s]); bw.put(xv, xb); put_tokens(bw, [], FIXED_LL, FIXED_D)
        yield case("distance_one_more_than_the_output_%s" % ("dynamic" if dyn else "fixed"), bw, bytes(body[:50]) + b"xxxxx")
    # a valid stream whose output is not ISIZE bytes long
    bw = BitWriter(); fixed_block(bw, good, 1)
    yield case("one_byte_too_many_by_a_literal", bw, want[:-1])
    t = body + [(30, 17)]
    bw = BitWriter(); fixed_block(bw, t, 1)
    yield case("one_byte_too_many_by_a_match", bw, expand(t)[:-1])
    bw = BitWriter(); dynamic_block(bw, t, 1, ll, d)
    yield case("one_byte_too_many_by_a_match_dynamic", bw, expand(t)[:-1])
    bw = BitWriter(); fixed_block(bw, body, 0); stored_block(bw, bytes(body), 1)
    yield case("one_byte_too_many_by_a_stored_block", bw, bytes(body + body)[:-1])
    bw = BitWriter(); fixed_block(bw, good, 1)
    yield case("end_of_block_one_byte_short", bw, want + b"x")
    bw = BitWriter(); dynamic_block(bw, good, 1, ll, d)
    yield case("end_of_block_one_byte_short_dynamic", bw, want + b"x")
    # large outputs too (the host decoder's fast loop runs while there are 274 bytes of room)
    big = pattern(300, 71) + [(258, 300)] * 20
    for delta in (-1, 1):
        for dyn in (0, 1):
            bw = BitWriter()
            if dyn: dynamic_block(bw, big, 1, ll, d)
            else: fixed_block(bw, big, 1)
            o = expand(big)
            yield case("large_output_isize_off_by_%+d_%s" % (delta, "dynamic" if dyn else "fixed"), bw, o[:-1] if delta < 0 else o + b"x")
    bw = BitWriter(); fixed_block(bw, good, 0)
    yield case("last_block_not_final", bw, want)
    bw = BitWriter(); stored_block(bw, bytes(body), 0)
    yield case("last_block_not_final_stored", bw, bytes(body))
    # input cut after every byte of the last 8 bytes of a valid stream
    for name, make in (("fixed", lambda b: fixed_block(b, good, 1)), ("dynamic", lambda b: dynamic_block(b, good, 1, ll, d)),
                       ("stored", lambda b: (fixed_block(b, good[:100], 0), stored_block(b, bytes(body[:20]), 1)))):
        bw = BitWriter(); make(bw)
        s = bw.bytes()
        o = want if name != "stored" else expand(good[:100]) + bytes(body[:20])
        assert judge(s, len(o)) == o
        for k in range(1, 9):
            yield case("%s_stream_cut_%d_bytes_short" % (name, k), s[:-k], o)
    # ISIZE 0 over a payload that is not an empty stream
    bw = BitWriter(); bw.put(1, 1); bw.put(3, 2); bw.put(0, 13)
    yield case("isize_0_over_block_type_3", bw, b"")
    bw = BitWriter(); fixed_block(bw, good, 1)
    yield case("isize_0_over_a_stream_with_output", bw, b"")
    yield case("isize_0_over_no_payload_at_all", b"", b"")
    bw = BitWriter(); fixed_block(bw, [], 0)
    yield case("isize_0_over_an_empty_block_that_is_not_final", bw, b"")


_CORPUS = None


def corpus():
    """Every case, valid and malformed (generated once per process; the assertions of Case run while it is)."""
    global _CORPUS
    if _CORPUS is None:
        cases = [c for g in VALID_GENERATORS for c in g()] + list(gen_malformed())
        names = [c.name for c in cases]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
        _CORPUS = cases
    return _CORPUS


def valid_cases():
    return [c for c in corpus() if c.valid]


def malformed_cases():
    return [c for c in corpus() if not c.valid]


def valid_file():
    """All valid cases as ONE BGZF file (the members that care start at their alignment), and its inflated bytes."""
    cs = valid_cases()
    return bgzf([(c.stream, c.intended) for c in cs], align=[c.align for c in cs]), b"".join(c.intended for c in cs)


def container(cases):
    """The corpus for tests/native/inflate_harness.cpp: per case u32 name length, name, u32 valid, u32 stream length, stream, u32 output
    length, the intended bytes; all little-endian."""
    out = bytearray()
    for c in cases:
        n = c.name.encode()
        out += struct.pack("<I", len(n)) + n + struct.pack("<II", 1 if c.valid else 0, len(c.stream)) + c.stream + struct.pack("<I", len(c.intended)) + c.intended
    return bytes(out)
