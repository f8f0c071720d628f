"""mpileup text with answers known by construction -- shared by tests/test_textgen.py (CPU) and
tests/test_gpu_mpileup_text_sizes.py (GPU).  Plain module, no fixtures.

A `Builder` composes mpileup text as BYTES from a seeded pool of base-string tokens.  Every token is put together from
pieces whose meaning is fixed when they are written down (a counted symbol, an ignored one, `^x`, an indel with its skipped
letters, a lone sign), so the counts of match / A / C / G / T a token holds are known without reading it back.  For every line
the builder records where each sample's base string lies and whether the reference's tokeniser loop processes it
(call_vC.cpp:490: only while something follows the tab that ends it, in the line stripped of its last character and cut at
a NUL).  `predict` applies the gates and the calling rule (call_vC.cpp:545-601) to the planted counts and renders the two
output files: a third, parser-free statement of the answer next to the oracle and the product.

The geometry helpers restate what the device parser's routes depend on (csrc/textcall.hip): `r` (offset of a line from the
16-byte boundary in front of it), the 1 KB steps of its tab scan and the 8192-byte LDS copy of a line."""
import random

import numpy as np

STEP = 1024            # bytes of a line the tab scan looks at per step
LDS = 8192             # bytes of a line (window bytes: counted from the aligned address in front of it) kept in LDS
TOK_CAP = 10000        # characters of a token the reference keeps
COUNTED = {c: k for k, cs in enumerate([b".,", b"aA", b"cC", b"gG", b"tT"]) for c in cs}      # byte -> class 0 match, 1-4 A C G T
IGNORED = b"*$Nn"
SKIPPED = b"ACGTNacgtn*"                        # letters behind +n / -n: counted symbols among them, which must NOT count
CARET_X = bytes(c for c in range(1, 256) if c not in (9, 10))     # `^x`: x is any byte but tab / newline / NUL
FOREIGN = b"<>RYKMxX#@ 0123456789" + bytes([0x80, 0xa7, 0xe9, 0xff])   # bytes the reference has no key for


INDEL_NS = (1, 1, 2, 3, 9, 12, 150)


def make_token(rnd, n_pieces, zero=False, indel_ns=INDEL_NS):
    """(token bytes, (match, A, C, G, T)) from n_pieces pieces of the legal alphabet; zero: no A / C / G / T is counted (they still
    occur as skipped letters and behind '^')."""
    out = bytearray()
    cnt = [0, 0, 0, 0, 0]
    for _ in range(n_pieces):
        u = rnd.random()
        if u < 0.60:
            c = rnd.choice(b".,.,.," if zero else b".,.,.,..,,ACGTacgtACGTacgt")
            out.append(c)
            cnt[COUNTED[c]] += 1
        elif u < 0.70:
            out.append(rnd.choice(IGNORED))
        elif u < 0.82:
            out.append(0x5e)
            out.append(rnd.choice(b"+-^ ]IATt.") if rnd.random() < 0.5 else rnd.choice(CARET_X))
        elif u < 0.94:
            n = rnd.choice(indel_ns)
            out.append(rnd.choice(b"+-"))
            out += (b"%0*d" % (rnd.choice([1, 1, 2, 3]), n))[-3:] if n < 100 else b"%d" % n       # 1-3 digits (leading zeros)
            out += bytes(rnd.choice(SKIPPED) for _ in range(n))
        elif u < 0.97:
            out += rnd.choice([b"+0", b"-0", b"-00"])
        else:
            out.append(rnd.choice(b"+-"))                                 # a sign without digits swallows nothing
    return bytes(out), tuple(cnt)


class Pool:
    """Tokens with their planted counts, ready to be put into a line: triple[i] = depth TAB token TAB quality."""

    def __init__(self, rnd, n, lens, zero=False, qual_cap=12, indel_ns=INDEL_NS):
        self.tok, self.triple, cnt, chars, boff = [], [], [], [], []
        # a sample without reads; a sample with one deleted base; a carrier of an individual call (T and G four times and more)
        fixed = [(b"", (0, 0, 0, 0, 0)), (b"*", (0, 0, 0, 0, 0)), (b"..TtTTT-2tt^Tgggg,*G", (3, 0, 0, 5, 5))]
        if zero:
            fixed.pop()
        for i in range(n):
            t, c = fixed[i] if i < len(fixed) else make_token(rnd, rnd.choice(lens), zero, indel_ns)
            assert len(t) <= TOK_CAP
            lead = b" " * rnd.randint(1, 3) if rnd.random() < 0.08 else b""          # toksplit skips leading blanks
            depth = b"%d" % sum(c)
            qual = b"" if rnd.random() < 0.1 else b"I" * min(len(t), qual_cap)
            self.tok.append(t)
            self.triple.append(depth + b"\t" + lead + t + b"\t" + qual)
            cnt.append(c)
            chars.append(len(t))
            boff.append((len(depth) + 1, len(depth) + 1 + len(lead) + len(t)))
        self.cnt, self.chars = cnt, chars
        self.boff = boff                                                  # (start of the base field, its ending tab) inside the triple
        self.tlen = [len(t) for t in self.triple]

    def __len__(self):
        return len(self.tok)


class Line:
    __slots__ = ("off", "raw_len", "stripped", "b", "e", "proc", "name", "pos", "refc", "cnt", "chars", "error", "n_fields")


class Text:
    """data: the bytes; S; lines: one Line per line of the file BEHIND the first; err_line: 1-based file line of the first planted
    domain error (None: well-formed)."""

    def __init__(self, data, S, lines):
        self.data, self.S, self.lines = data, S, lines
        bad = [i + 2 for i, ln in enumerate(lines) if ln.error]
        self.err_line = bad[0] if bad else None
        self.base_chars = int(sum(int(ln.chars[ln.proc].sum()) for ln in lines if ln.b is not None and len(ln.b)))
        self.n_lines = len(lines) + 1 if data else 0

    def r_of(self, i):
        """r of lines[i] when the whole text goes through one launch: the chunk starts at the file's second line on a 256-byte
        boundary."""
        return (self.lines[i].off - self.lines[0].off) % 16


NAMES = [(b"c1", b"c1"), (b"c1", b"c1"), (b"ctg.x", b"ctg.x"), (b" c3", b"c3"), (b"k\xe9\xffz", b"k\xe9\xffz")]     # (field, printed)
REFS = [(b"A", 65), (b"C", 67), (b"G", 71), (b"T", 84), (b"N", 78), (b"a", 97), (b"c", 99), (b"g", 103), (b"t", 116), (b"", 0), (b"AC", 65), (b" T", 84)]


class Builder:
    def __init__(self, seed, S, lens=(0, 0, 1, 3, 8, 20, 60), pool=600, qual_cap=12, indel_ns=INDEL_NS):
        self.rnd = random.Random(seed)
        self.S = S
        self.pool = Pool(self.rnd, pool, lens, qual_cap=qual_cap, indel_ns=indel_ns)
        self.zero = Pool(self.rnd, max(40, pool // 6), lens, zero=True, qual_cap=qual_cap, indel_ns=indel_ns)
        self.parts, self.lines, self.off = [], [], 0
        self._emit(self._compose(self._header(0), [(self.pool, 0)] * S)[0])            # the first line: S samples, never processed

    # ---- pieces
    def _header(self, lineno, plain=False):
        rnd = self.rnd
        name = NAMES[0] if plain else rnd.choice(NAMES)
        u = 1.0 if plain else rnd.random()
        pos = (b" 7", 7) if u < 0.02 else (b"12x", 12) if u < 0.04 else (b"-3", -3) if u < 0.05 else (b"", 0) if u < 0.06 else (b"%d" % lineno, lineno)
        refc = REFS[0] if plain else rnd.choice(REFS)
        return name, pos, refc

    def _compose(self, header, picks, extra_qual=0):
        """header + one triple per (pool, index) pick; extra_qual lengthens the last quality field."""
        name, pos, refc = header
        head = name[0] + b"\t" + pos[0] + b"\t" + refc[0]
        fields = [head] + [p.triple[i] for p, i in picks]
        body = b"\t".join(fields) + b"I" * extra_qual
        n = len(picks)
        if n:
            tl = np.array([p.tlen[i] for p, i in picks], dtype=np.int64)
            start = len(head) + 1 + np.concatenate(([0], np.cumsum(tl[:-1] + 1)))
            bo = np.array([p.boff[i] for p, i in picks], dtype=np.int64)
            b, e = start + bo[:, 0], start + bo[:, 1]
            cnt = np.array([p.cnt[i] for p, i in picks], dtype=np.int64)
            chars = np.array([p.chars[i] for p, i in picks], dtype=np.int64)
            assert body[int(e[-1])] == 9 and (int(b[-1]) == 0 or body[int(b[-1]) - 1] == 9)
        else:
            b = e = chars = np.zeros(0, np.int64)
            cnt = np.zeros((0, 5), np.int64)
        return body, b, e, cnt, chars

    def _emit(self, body, newline=True, rec=None):
        raw = body + (b"\n" if newline else b"")
        if rec is not None:
            rec.off, rec.raw_len = self.off, len(raw)
            self.lines.append(rec)
        self.parts.append(raw)
        self.off += len(raw)

    def _record(self, header, body, b, e, cnt, chars, newline, nul_at=None, error=False):
        """What the reference sees of the line: cut at the first NUL, then its last character dropped (the newline, if there is
        one); base string s is processed if the tab at e[s] is followed by at least one more character."""
        ln = Line()
        seen = len(body) + (1 if newline else 0)
        if nul_at is not None:
            seen = min(seen, nul_at)
        ln.stripped = max(0, seen - 1)
        ln.b, ln.e = b, e
        ln.proc = (e + 1 < ln.stripped) if len(e) else np.zeros(0, bool)
        ln.name, ln.pos, ln.refc = header[0][1], header[1][1], header[2][1]
        ln.cnt, ln.chars, ln.error = cnt, chars, error
        return ln

    # ---- lines
    def line(self, m=None, hot=None, trailing_tab=False, newline=True, pad_to=None, picks=None, nul_at=None, plain=False,
             bad_at=None, extra=0, tail=b""):
        """One line of m samples (default S; S + extra plants the reference's out-of-bounds write).  hot = (lo, hi): only the
        samples lo <= s < hi draw tokens that count A / C / G / T, the others draw from the zero pool.  pad_to: the raw line (with its
        newline) gets exactly this many bytes (the last quality field grows).  nul_at: a NUL replaces that byte of the line.
        bad_at = (sample, byte): that sample's base string gets `byte` (no key in the reference) in front."""
        rnd = self.rnd
        m = (self.S if m is None else m) + extra
        header = self._header(len(self.lines) + 2, plain)
        if picks is None:
            idx = [rnd.randrange(len(self.pool)) for _ in range(m)]
            if hot is None:
                picks = [(self.pool, i) for i in idx]
            else:
                picks = [(self.pool, i) if hot[0] <= s < hot[1] else (self.zero, i % len(self.zero)) for s, i in enumerate(idx)]
        body, b, e, cnt, chars = self._compose(header, picks)
        if trailing_tab:
            body += b"\t"
        body += tail                                                      # (a started field that no tab ends: never processed)
        if pad_to is not None:
            need = pad_to - len(body) - (1 if newline else 0)
            assert need >= 0 and not trailing_tab, (pad_to, len(body))
            body += b"I" * need
        if bad_at is not None:
            s, byte = bad_at
            assert e[s] > b[s] and byte != 0x20, "the foreign byte needs a token to sit in, and a leading blank would be skipped"
            body = body[:b[s]] + bytes([byte]) + body[b[s] + 1:]
        if nul_at is not None:
            if callable(nul_at):
                nul_at = nul_at(b, e)
            assert nul_at < len(body)
            body = body[:nul_at] + b"\0" + body[nul_at + 1:]
        rec = self._record(header, body, b, e, cnt, chars, newline, nul_at)
        rec.error = bool(rec.proc[self.S:].any()) or (bad_at is not None and bool(rec.proc[bad_at[0]]))
        self._emit(body, newline, rec)
        return rec

    def raw(self, body, newline=True):
        """A hand-made line that holds no processed base string (an empty line, a cut header ...)."""
        rec = self._record(((b"", b""), (b"", 0), (b"", 0)), body, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 5), np.int64),
                           np.zeros(0, np.int64), newline)
        self._emit(body, newline, rec)
        return rec

    def custom(self, toks, quals=None, newline=True, plain=True, nul_at=None):
        """A line of hand-written tokens: toks = [(token bytes, (match, A, C, G, T), characters processed)]."""
        p = Pool.__new__(Pool)
        p.tok, p.triple, cnt, chars, boff = [], [], [], [], []
        for k, (t, c, nch) in enumerate(toks):
            q = quals[k] if quals else b"I"
            p.triple.append(b"1\t" + t + b"\t" + q)
            cnt.append(c); chars.append(nch); boff.append((2, 2 + len(t)))
        p.cnt, p.chars, p.boff = cnt, chars, boff
        p.tlen = [len(t) for t in p.triple]
        return self.line(picks=[(p, k) for k in range(len(toks))], newline=newline, plain=plain, nul_at=nul_at)

    def align_next(self, r, m=1):
        """A short line padded so that the NEXT line starts r bytes behind a 16-byte boundary (counted from the file's second line)."""
        base = self.lines[0].off if self.lines else self.off
        short = next(i for i in range(2, len(self.pool)) if self.pool.tlen[i] < 100)
        for pad in range(200, 216):
            if (self.off + pad - base) % 16 == r:
                return self.line(picks=[(self.pool, short)] * min(m, self.S), pad_to=pad)

    def text(self):
        return Text(b"".join(self.parts), self.S, self.lines)


# ---------------------------------------------------------------- the answer, from the planted counts alone
def predict(text, c=4, t=4, p=0.01):
    """(called_SNPs, indiv_called) as bytes, or None where the reference meets a planted domain error first.  Gates
    call_vC.cpp:545-552, calling rule :577-601 (alleles in the order a c t g; the allele that equals the reference CHARACTER is
    skipped), line layout :641-667."""
    if text.err_line is not None:
        return None
    S = text.S
    pop_out, ind_out = [], []
    for ln in text.lines:
        if not ln.proc.any():
            continue
        cnt = np.zeros((S, 5), np.int64)
        k = min(S, len(ln.proc))
        cnt[:k] = ln.cnt[:k] * ln.proc[:k, None]
        tot = cnt.sum(0).tolist()
        cov = sum(tot)
        if cov < c or cov - tot[0] < t:
            continue
        pop, ind = [], []
        for x, lower in ((1, 97), (2, 99), (4, 116), (3, 103)):
            if lower == ln.refc:
                continue
            n = tot[x]
            col = cnt[:, x]
            if n >= t and float(n) >= cov * p:
                dst = pop
            elif (col >= t).any():
                dst = ind
            else:
                continue
            dst.append(b"%d|%c|.|" % (n, lower - 32) + b"|".join(map(b"%d".__mod__, col.tolist())))
        covs = b"|".join(map(b"%d".__mod__, cnt.sum(1).tolist()))
        head = ln.name + b"\t-\t%d\t" % ln.pos + bytes([ln.refc]) + b"\t" + covs + b"\t"
        if pop:
            pop_out.append(head + b",".join(pop) + b"\n")
        if ind:
            ind_out.append(head + b",".join(ind) + b"\n")
    return b"".join(pop_out), b"".join(ind_out)


# ---------------------------------------------------------------- geometry of the device parser's routes, from the layout alone
def routes(text):
    """What the text reaches, as a dict of sets / counts (window byte j of a line = line byte j - r)."""
    out = {"r_long": set(), "step_straddle_k": set(), "lds_straddle": 0, "lds_behind": 0, "tabs_in_two_steps": 0, "proc_max": 0}
    for i, ln in enumerate(text.lines):
        r = text.r_of(i)
        if ln.raw_len > STEP:
            out["r_long"].add(r)
        if not ln.proc.any():
            continue
        b, e = ln.b[ln.proc] + r, ln.e[ln.proc] + r                      # window coordinates of the processed base strings
        out["proc_max"] = max(out["proc_max"], int(ln.proc.nonzero()[0].max()) + 1)
        for k in np.unique(e // STEP):
            if k > 0 and ((b < k * STEP) & (e > k * STEP)).any():
                out["step_straddle_k"].add(int(k))
        out["lds_straddle"] += int(((b < LDS) & (e > LDS)).sum())
        out["lds_behind"] += int((b >= LDS).sum())
        out["tabs_in_two_steps"] += int((((b - 1) // STEP) != (e // STEP)).sum())
    return out


def both_directions(text, grid, min_lines=16):
    """Of the wavefronts of a `grid`-wavefront launch over the whole text (line i of the chunk goes to wavefront i % grid) that
    handle at least min_lines lines: how many see the number of processed samples fall from one of their lines to the next AND
    rise again, and how many such wavefronts there are."""
    n = np.array([int(ln.proc.sum()) for ln in text.lines])
    both = total = 0
    for w in range(min(grid, len(n))):
        seq = n[w::grid]
        if len(seq) < min_lines:
            continue
        d = np.diff(seq)
        total += 1
        both += bool((d < 0).any() and (d > 0).any())
    return both, total


# ---------------------------------------------------------------- the shapes (both test files build the same texts)
SAMPLE_COUNTS = [63, 64, 65, 128, 129, 511, 512, 513, 600, 1100]


def shape_samples(S, n_lines=160, seed=0):
    """Shape 1: S samples; the counted A / C / G / T sit in all samples, in s >= 64, in s >= 512 (or the upper half) and in the
    LAST sample in turn; some lines end early, carry a trailing tab or samples without reads."""
    bl = Builder(1000 + S + seed, S, lens=(0, 0, 1, 3, 8, 12), pool=400, qual_cap=4)
    hi = 512 if S > 512 else S // 2
    zero = lambda: [(bl.zero, bl.rnd.randrange(len(bl.zero))) for _ in range(S)]
    for i in range(n_lines):
        mode = i % 8
        if mode == 0:
            bl.line()
        elif mode == 1:
            bl.line(hot=(min(64, S - 1), S))
        elif mode == 2 and i % 16 == 2:
            bl.line(hot=(hi, S))
        elif mode == 2:
            picks = zero()
            picks[hi] = (bl.pool, 2)                                      # only sample hi + 1 (513 of more than 512) carries the call
            bl.line(picks=picks)
        elif mode == 3:
            picks = zero()
            picks[S - 1] = (bl.pool, 2)                                   # only the last sample does; the trailing tab has it processed
            bl.line(picks=picks, trailing_tab=True)
        elif mode == 4:
            bl.line(m=bl.rnd.randint(0, S))                              # samples missing at the end of the line
        elif mode == 5:
            bl.line(hot=(S - 1, S))                                      # ... here it is processed only if its quality field is not empty
        elif mode == 6:
            bl.line(hot=(S - 2, S - 1))
        else:
            bl.line(hot=(0, 1))
    return bl.text()


def shape_documented(n_lines=2400, seed=0):
    """Shape 2: the shape KERNELS.md quotes the kernel at -- 160 samples, lines of about 4 KB."""
    bl = Builder(2000 + seed, 160, lens=(0, 1, 3, 5, 8, 8, 12, 20), pool=1500, qual_cap=8, indel_ns=(1, 1, 1, 2, 2, 3, 3, 9, 12, 1, 2, 3, 1, 2, 30, 150))
    for i in range(n_lines):
        bl.line(m=None if i % 11 else bl.rnd.randint(100, 160))
    return bl.text()


def _long_line(bl, pools, target, r, plain=False, nul_at=None):
    """A line of exactly `target` raw bytes that starts r bytes behind a 16-byte boundary: tokens are drawn while they fit, the
    samples that no longer fit stay without reads, the last quality field takes up the rest."""
    bl.align_next(r)
    rnd, S = bl.rnd, bl.S
    budget = target - 60 - 4 * S                                          # (a sample without reads: "0", two empty fields, three tabs)
    picks = []
    for s in range(S):
        p = rnd.choice(pools)
        i = rnd.randrange(2, len(p))
        if p.tlen[i] - 3 <= budget and rnd.random() < 0.85:
            budget -= p.tlen[i] - 3
            picks.append((p, i))
        else:
            picks.append((bl.pool, 0))
    return bl.line(picks=picks, pad_to=target, plain=plain, nul_at=nul_at)


def shape_long(seed=0):
    """Shape 3: lines of 1 KB +- 16, 2 KB, 8 KB +- 32 and 20-100 KB at all 16 alignments, with tokens of up to a few KB."""
    bl = Builder(3000 + seed, 48, lens=(1, 3, 8, 20), pool=200)
    mid = Pool(bl.rnd, 200, (20, 60, 120, 200))
    big = Pool(bl.rnd, 120, (200, 400, 900, 1500, 1500))
    rnd = bl.rnd
    for r in range(16):
        _long_line(bl, [bl.pool], 1024 - 16 + 2 * r + rnd.randint(0, 1), r)
        _long_line(bl, [bl.pool, mid], 2048 - r, r)
        _long_line(bl, [mid, big], 8192 - 32 + 4 * r + rnd.randint(0, 3), r)
        _long_line(bl, [mid, big], 8192 - r + 1, r)                       # the newline is the last byte of the LDS copy
        _long_line(bl, [mid, big, big], rnd.randint(20000, 100000), r)
    bl.line(newline=False)
    return bl.text()


def shape_cut(seed=0):
    """Shape 3: tokens longer than the 10 000 characters toksplit keeps, on a line that also holds 200 other samples: what lies
    behind the cut neither counts nor is skipped by an indel announced in front of it."""
    bl = Builder(3100 + seed, 202, lens=(0, 1, 3, 8, 20), pool=300)
    deep = (b"." * 9990 + b"TTTTTTTTTT" + b"GGGGGGGG", (9990, 0, 0, 0, 10), TOK_CAP)
    deep2 = (b"  " + b"," * 9996 + b"+9ACGTACGTA" + b"tttt", (9996, 0, 0, 0, 0), TOK_CAP)
    p = Pool.__new__(Pool)
    p.triple = [b"9\t" + deep[0] + b"\tI", b"9\t" + deep2[0] + b"\t"]
    p.cnt, p.chars = [deep[1], deep2[1]], [TOK_CAP, TOK_CAP]
    p.boff = [(2, 2 + len(deep[0])), (2, 2 + len(deep2[0]))]
    p.tlen = [len(t) for t in p.triple]
    for at in ((0, 150), (100, 201), (63, 64), (201, 7)):
        for r in (0, 9):
            bl.align_next(r)
            picks = [(bl.pool, bl.rnd.randrange(len(bl.pool))) for _ in range(202)]
            picks[at[0]], picks[at[1]] = (p, 0), (p, 1)
            bl.line(picks=picks, trailing_tab=True)
    return bl.text()


def shape_insertion_over_the_edge(seed=0):
    """Shape 3: a `+150` insertion announced in front of window byte 8192 whose 150 skipped letters end behind it (the token is
    read from memory as a whole), at several alignments and distances; the letters behind the insertion count."""
    bl = Builder(3200 + seed, 6, lens=(1, 3, 8))
    ins = b"..,," + b"+150" + bytes(bl.rnd.choice(SKIPPED) for _ in range(150)) + b"TTTTT" + b"-2ac" + b"gG"
    for r in (0, 1, 7, 15):
        for back in (1, 4, 60, 149, 153):                                 # the '+' sits `back` window bytes in front of the edge
            bl.align_next(r)
            # "c1" TAB line TAB "A" TAB | "1" TAB "..." TAB q0 TAB | "1" TAB "..,," "+150"
            q0 = b"I" * (LDS - back - r - 4 - 2 - 13 - len(b"%d" % (len(bl.lines) + 2)))
            rec = bl.custom([(b"...", (3, 0, 0, 0, 0), 3), (ins, (4, 0, 0, 2, 5), len(ins)), (b"AAAA", (0, 4, 0, 0, 0), 4)], quals=[q0, b"II", b"I"])
            plus = int(rec.b[1]) + 4 + r
            assert plus == LDS - back and plus + 4 + 150 > LDS, plus
    return bl.text()


def shape_most_samples(S=16383, seed=0):
    """Shape 3: the most samples the product takes, four lines behind the first."""
    bl = Builder(3300 + seed, S, lens=(0, 1, 1, 2), pool=64, qual_cap=1)
    bl.line()
    bl.line(hot=(S - 1, S), trailing_tab=True)
    bl.line(m=S - 5000)
    bl.line(hot=(512, S))
    return bl.text()


def shape_many_lines(n_lines=50000, seed=0):
    """Shape 4: many lines per wavefront in one launch; the kind of a line is drawn, so that whatever the grid, the lines one
    wavefront takes one after the other hold now more, now fewer processed samples than the one before."""
    bl = Builder(4000 + seed, 130, lens=(0, 1, 1, 2, 3, 5), pool=500, qual_cap=2)
    rnd = bl.rnd
    for _ in range(n_lines):
        u = rnd.random()
        if u < 0.30:
            bl.line(m=3)                                                  # 3 samples' worth of tabs on a line of a 130-sample file
        elif u < 0.45:
            bl.line()
        elif u < 0.60:
            bl.raw(b"")
        elif u < 0.72:
            bl.line(m=1, picks=[(bl.pool, rnd.randrange(2, 500))])         # cut behind field 5: its base string has no tab behind it ...
        elif u < 0.80:
            bl.line(m=1, trailing_tab=True)
        elif u < 0.88:
            bl.line(m=rnd.randint(60, 129))
        elif u < 0.94:
            bl.line(m=rnd.randint(4, 70), trailing_tab=True)
        elif u < 0.97:
            bl.raw(rnd.choice([b"c1", b"c1\t77", b"c1\t78\tA", b"c1\t79\tA\t3", b"\t\t\t"]))
        else:
            bl.line(m=rnd.randint(2, 100), tail=rnd.choice([b"\t7\t", b"\t7\tTTTTTTT", b"\t4\t,,,,"]))   # cut inside the next sample's base string
    return bl.text()


def _nul_base(seed):
    bl = Builder(5000 + seed, 5, lens=(1, 3, 8, 20), pool=200)
    mid = Pool(bl.rnd, 100, (20, 60, 120, 200, 400))
    return bl, mid


NUL_CASES = ["name", "in_token", "behind_tab_1", "behind_tab_2", "behind_tab_3", "first_byte", "b1023_r0", "b1024_r0", "b1025_r0",
             "b8191_r0", "b8192_r0", "b1023_r5", "b1024_r5", "b1025_r5", "b8191_r5", "b8192_r5", "w1024_r5", "w8192_r5"]


def shape_nul(case, seed=0):
    """Shape 5: one NUL in an otherwise well-formed text.  The reference's strlen ends the line there and the character in front
    of the NUL is the one that is dropped; the lines around it are untouched."""
    bl, mid = _nul_base(seed)
    for _ in range(6):
        bl.line()
    if case == "name":
        bl.line(nul_at=1, plain=True)
    elif case == "first_byte":
        bl.line(nul_at=0, plain=True)
    elif case in ("in_token", "behind_tab_1", "behind_tab_2", "behind_tab_3"):
        tk = [(b"TTTTcc..,", (3, 0, 2, 0, 4), 9)] * 5
        at = (lambda b, e: int(b[2]) + 4) if case == "in_token" else (lambda b, e: int(e[2]) + int(case[-1]))
        bl.custom(tk, quals=[b"IIIIIIIII"] * 5, nul_at=at)
    else:
        where, r = case.split("_")
        r = int(r[1:])
        _long_line(bl, [bl.pool, mid], 9000, r, plain=True, nul_at=int(where[1:]) - (r if where[0] == "w" else 0))   # b: byte of the line; w: of the window
    for _ in range(5):
        bl.line()
    return bl.text()


def shape_foreign(kind, seed=0):
    """Shape 5: bytes >= 0x80 -- behind '^' they are a mapping quality like any other; as a symbol the reference has no key for
    them."""
    bl = Builder(5100 + seed, 70, lens=(1, 3, 8, 20), pool=300)
    for i in range(40):
        bl.line()
    if kind == "caret":
        hi = [(b"^" + bytes([x]) + b"T" * 4, (0, 0, 0, 0, 4), 6) for x in (0x80, 0x9c, 0xc3, 0xff, 0x7f, 0x01)]
        bl.custom(hi * 11 + hi[:4])
    else:
        byte = {"symbol_80": 0x80, "symbol_ff": 0xff, "symbol_digit": 0x37, "symbol_R": 0x52}[kind]
        picks = [(bl.pool, bl.rnd.randrange(2, len(bl.pool))) for _ in range(70)]
        while bl.pool.chars[picks[66][1]] == 0:
            picks[66] = (bl.pool, bl.rnd.randrange(2, len(bl.pool)))
        bl.line(picks=picks, bad_at=(66, byte))
    for i in range(10):
        bl.line()
    return bl.text()


def shape_which_error(bad_lines=(40, 7000, 31000), extra_line=12000, both_line=None, n_lines=32000, seed=0):
    """Shape 6: a 3-sample text with foreign symbols on the given (1-based) file lines, one sample too many on extra_line, and
    (both_line) a line that holds both.  Returns (Text, {file line: planted byte})."""
    bl = Builder(6000 + seed, 3, lens=(1, 3, 8), pool=200)
    planted = {}
    for fl in range(2, n_lines + 1):
        picks = [(bl.pool, bl.rnd.randrange(2, len(bl.pool))) for _ in range(3)]
        if fl in bad_lines or fl == both_line:
            while bl.pool.chars[picks[1][1]] == 0:
                picks[1] = (bl.pool, bl.rnd.randrange(2, len(bl.pool)))
            byte = [x for x in FOREIGN if x != 0x20][fl % (len(FOREIGN) - 1)]
            planted[fl] = byte
            if fl == both_line:
                picks.append((bl.pool, 3))
            bl.line(picks=picks, bad_at=(1, byte), trailing_tab=fl == both_line)
            assert bl.lines[-1].error
        elif fl == extra_line:
            picks.append((bl.pool, 3))
            bl.line(picks=picks, trailing_tab=True)
            assert bl.lines[-1].error
        else:
            bl.line(picks=picks)
    return bl.text(), planted


def keep_until(text, file_line):
    """The Text of the lines in front of (1-based) file_line, error marks dropped: what the reference has written when it stops there."""
    lines = text.lines[:file_line - 2]
    t = Text(text.data[:text.lines[file_line - 2].off], text.S, lines)
    t.err_line = None
    return t


WELL_FORMED = {}
for _S in SAMPLE_COUNTS:
    WELL_FORMED["samples_%d" % _S] = (lambda S=_S: shape_samples(S))
WELL_FORMED.update({"documented": shape_documented, "long": shape_long, "cut": shape_cut, "insertion": shape_insertion_over_the_edge,
                    "most_samples": shape_most_samples, "many_lines": shape_many_lines, "foreign_caret": lambda: shape_foreign("caret")})
for _c in NUL_CASES:
    WELL_FORMED["nul_" + _c] = (lambda c=_c: shape_nul(c))
SETTINGS = [dict(c=1, t=1, p=0.0), dict(c=4, t=4, p=0.01), dict(c=30, t=3, p=0.2)]
