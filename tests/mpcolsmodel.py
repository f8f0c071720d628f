"""A pure-Python model of what `samtools mpileup -a / -aa`, `-s` and `-O` add to the text (include/msnv.h msnv_mpileup_text_opts), for the
tests of those options: the oracle (oracle/orc_mpileup.c) knows none of the three, so the expected text is its text plus what this
module derives.

  columns()      a plain pileup of UNPAIRED reads: per line and sample the kept elements' count, quality string, MAPQ string and read
                 offsets.  CIGAR M I D N S H P = X, the read filters, -Q.  No mates edit, no depth cap.
  add_columns()  a text without the extra columns -> the text with them, the values from columns()
  fill_all()     a text without zero-depth lines -> the text of -a / -aa

tests/test_mpcols_model.py pins columns() on the oracle (cnt and qualities, which the oracle prints) and fill_all() on a literal."""
from bamtools import iter_records

M, I, D, N, S, H, P, EQ, X = range(9)
REF_OPS = (M, D, N, EQ, X)


def _regions(bed):
    return {t: (b, e) for t, b, e in (bed or [])}


def _pushed(names, seqs, sample, bed, flag_filter, min_mapq, count_orphans):
    """The reads of one sample that reach the pileup (bam_plcmd.c mplp_func), in file order: (tid, pos, end, record)."""
    reg = _regions(bed)
    for r in iter_records(sample):
        rlen = sum(n for n, op in r["cigar"] if op in REF_OPS)
        end = r["pos"] + rlen
        if r["tid"] < 0 or r["flag"] & 4 or r["flag"] & flag_filter:
            continue
        if bed is not None and bed != []:
            if r["tid"] not in reg or not (reg[r["tid"]][0] < max(end, r["pos"] + 1) and r["pos"] < reg[r["tid"]][1]):
                continue
        if seqs is not None and seqs[r["tid"]] is not None and len(seqs[r["tid"]]) <= r["pos"]:
            continue
        if r["mapq"] < min_mapq or (not count_orphans and r["flag"] & 1 and not r["flag"] & 2) or rlen == 0:
            continue
        yield r["tid"], r["pos"], end, r


def pushed_tids(names, seqs, samples, bed=None, flag_filter=0x704, min_mapq=0, count_orphans=0):
    """The contigs that hold a read which reaches the pileup."""
    return {t for s in samples for t, _, _, _ in _pushed(names, seqs, s, bed, flag_filter, min_mapq, count_orphans)}


def _elements(r):
    """(reference position, qpos, is deletion or ref-skip) of every pileup element of one read: qpos of a D / N element is the count of
    read bases consumed before it (sam.c resolve_cigar2)."""
    x, y = r["pos"], 0
    for n, op in r["cigar"]:
        if op in (M, EQ, X):
            for k in range(n):
                yield x + k, y + k, False
            x += n
            y += n
        elif op in (D, N):
            for k in range(n):
                yield x + k, y, True
            x += n
        elif op in (I, S):
            y += n


def columns(names, lengths, seqs, samples, min_baseq, bed=None, flag_filter=0x704, min_mapq=0, count_orphans=0):
    """{(tid, pos0): [per sample (cnt, quality string, MAPQ string, [qpos + 1, ...])]} for every line of the text; a cell without kept
    elements is (0, "*", "*", [])."""
    n_s = len(samples)
    cells = {}
    reg = _regions(bed)
    for s, sample in enumerate(samples):
        for tid, pos, end, r in _pushed(names, seqs, sample, bed, flag_filter, min_mapq, count_orphans):
            l_seq = len(r["qual"])
            for p, qpos, _ in _elements(r):
                if bed and not (reg[tid][0] <= p < reg[tid][1]):
                    continue
                line = cells.setdefault((tid, p), [[] for _ in range(n_s)])
                q = r["qual"][qpos] if qpos < l_seq else 0
                if q >= min_baseq:
                    line[s].append((chr(min(q + 33, 126)), chr(min(r["mapq"] + 33, 126)), qpos + 1))
    out = {}
    for key, line in cells.items():
        out[key] = [(len(c), "".join(e[0] for e in c) or "*", "".join(e[1] for e in c) or "*", [e[2] for e in c]) for c in line]
    return out


def add_columns(text, names, cols, mq, bp):
    """text: lines `name pos REF {cnt bases quals}`; the same lines with the MQ and / or BP column of cols behind every cell's qualities."""
    tid_of = {n: i for i, n in enumerate(names)}
    out = []
    for ln in text.split("\n")[:-1]:
        f = ln.split("\t")
        cells = cols[(tid_of[f[0]], int(f[1]) - 1)]
        g = f[:3]
        for s in range((len(f) - 3) // 3):
            cnt, quals, mqs, bps = cells[s]
            assert int(f[3 + 3 * s]) == cnt and f[5 + 3 * s] == quals, (ln, s, cells[s])
            g += f[3 + 3 * s:6 + 3 * s]
            if mq:
                g.append(mqs)
            if bp:
                g.append(",".join(str(v) for v in bps) or "*")
        out.append("\t".join(g))
    return "".join(l + "\n" for l in out)


def strip_columns(text, n_extra):
    """The text without the n_extra columns behind every cell's qualities, and the stripped columns: [(line, sample, cnt, quals, extras)]."""
    out, taken = [], []
    w = 3 + n_extra
    for k, ln in enumerate(text.split("\n")[:-1]):
        f = ln.split("\t")
        assert (len(f) - 3) % w == 0, ln
        g = f[:3]
        for s in range((len(f) - 3) // w):
            c = f[3 + w * s:3 + w * (s + 1)]
            g += c[:3]
            taken.append((k, s, int(c[0]), c[2], c[3:]))
        out.append("\t".join(g))
    return "".join(l + "\n" for l in out), taken


def fill_all(default_text, names, lengths, seqs, bed, S, n_extra, level):
    """The zero-depth lines of -a (level 1) / -aa (level 2) put into default_text: for every contig in play -- one with a line in
    default_text, or with -aa every contig -- a line `name pos REF {0 * * [*]...}` for every position 1 .. length, cut to the
    contig's BED region when there is a BED, that has no line yet.  Order: tid, then position."""
    tid_of = {n: i for i, n in enumerate(names)}
    have = {}
    for ln in default_text.split("\n")[:-1]:
        f = ln.split("\t", 2)
        have.setdefault(tid_of[f[0]], {})[int(f[1]) - 1] = ln
    reg = _regions(bed)
    cell = "\t0\t*\t*" + "\t*" * n_extra
    out = []
    for tid, name in enumerate(names):
        lines = have.get(tid, {})
        if level == 0 or (level == 1 and not lines):
            out += [lines[p] for p in sorted(lines)]
            continue
        lo, hi = 0, lengths[tid]
        if bed:
            lo, hi = (max(reg[tid][0], 0), min(reg[tid][1], hi)) if tid in reg else (0, 0)
        seq = seqs[tid] if seqs is not None else None
        for p in sorted(set(lines) | set(range(lo, hi))):
            out.append(lines[p] if p in lines else "%s\t%d\t%s%s" % (name, p + 1, seq[p] if seq is not None and p < len(seq) else "N", cell * S))
    return "".join(l + "\n" for l in out)
