"""tests/mpcolsmodel.py is the yardstick of the mpileup options the oracle does not know (-a / -aa, -s, -O;
tests/test_gpu_mpileup_columns.py).  Before it judges the kernels it is pinned here, without a device: what columns() shares with the
oracle's text -- which lines exist, every cell's count and quality string -- equals the oracle on seeded random unpaired cohorts, and
fill_all() gives the literal text of a hand-placed case."""
import random

import orc
from bamtools import make_record as R, records
from mpcolsmodel import add_columns, columns, fill_all, pushed_tids, strip_columns


def random_cigar(rnd, max_ref=40):
    """(CIGAR string, read bases it consumes): [H] [S] [I] match { I | D | N | P I | P } match ... [S] [H]."""
    ops, l_seq = [], 0
    if rnd.random() < 0.15:
        ops.append("%dH" % rnd.randrange(1, 5))
    if rnd.random() < 0.25:
        n = rnd.randrange(1, 6); ops.append("%dS" % n); l_seq += n
    if rnd.random() < 0.1:
        n = rnd.randrange(1, 4); ops.append("%dI" % n); l_seq += n
    for k in range(rnd.randrange(1, 5)):
        if k:
            kind = rnd.choice("IIDDNP")
            n = rnd.randrange(1, 12 if kind in "DN" else 4)
            if kind == "P":
                ops.append("%dP" % n)
                if rnd.random() < 0.7:
                    n = rnd.randrange(1, 4); ops.append("%dI" % n); l_seq += n
            else:
                ops.append("%d%s" % (n, kind))
                if kind == "I":
                    l_seq += n
        n = rnd.randrange(1, max_ref // 3)
        ops.append("%d%s" % (n, rnd.choice("MMMM=X"))); l_seq += n
    if rnd.random() < 0.25:
        n = rnd.randrange(1, 6); ops.append("%dS" % n); l_seq += n
    if rnd.random() < 0.15:
        ops.append("%dH" % rnd.randrange(1, 5))
    return "".join(ops), l_seq


def random_cohort(rnd, n_samples=None, n_contigs=None, max_len=260, reads=40, max_ref=40):
    """Unpaired reads (flag: strand, and now and then a bit the filters look at), MAPQ 0..255, some reads with `*` qualities (0xff) and
    some without SEQ, on contigs of which one may lack its FASTA record and one may have a FASTA shorter than its length."""
    n_contigs = n_contigs or rnd.randrange(1, 4)
    names = ["k%d" % i for i in range(n_contigs)]
    lengths = [rnd.randrange(30, max_len) for _ in names]
    seqs = []
    for L in lengths:
        u = rnd.random()
        seqs.append(None if u < 0.15 else "".join(rnd.choice("ACGTacgtN") for _ in range(L if u < 0.85 else rnd.randrange(1, L))))
    samples = []
    for _ in range(n_samples or rnd.randrange(1, 5)):
        recs = []
        for i in range(rnd.randrange(0, reads)):
            tid = rnd.randrange(n_contigs)
            cigar, l_seq = random_cigar(rnd, max_ref)
            pos = rnd.randrange(0, lengths[tid])
            u = rnd.random()
            if u < 0.08:
                seq, qual = "*", []
            else:
                seq = "".join(rnd.choice("ACGTN=") for _ in range(l_seq))
                qual = [255] * l_seq if u < 0.16 else [rnd.choice([0, 5, 12, 13, 14, 30, 40, 92, 93, 94, 200]) for _ in range(l_seq)]
            flag = rnd.choice([0, 16]) | rnd.choice([0] * 12 + [0x400, 0x100, 0x200, 4])
            recs.append((tid, pos, i, R(tid, pos, cigar, seq, qual, flag=flag, mapq=rnd.choice([0, 1, 60, 92, 93, 94, 255, rnd.randrange(256)]), name="r%d" % i)))
        recs.sort(key=lambda t: t[:3])
        samples.append(records(*[r[3] for r in recs]))
    return names, lengths, seqs, samples


def test_columns_equal_the_oracle_where_the_oracle_speaks():
    rnd = random.Random(20241019)
    n_lines = n_noseq = 0
    for case in range(200):
        names, lengths, seqs, samples = random_cohort(rnd)
        if case % 5 == 4:
            seqs = None
        mp = dict(min_baseq=rnd.choice([0, 13, 13, 31]), flag_filter=rnd.choice([0x704, 0x704, 0x400, 0]), min_mapq=rnd.choice([0, 0, 1, 61]))
        bed = None
        if case % 4 == 3:
            bed = [(t, rnd.randrange(0, 20), lengths[t] - rnd.randrange(0, 20)) for t in range(len(names)) if rnd.random() < 0.7] or [(0, 3, 9)]
        text = orc.mpileup_text(names, lengths, seqs, samples, bed=bed, mp=mp)
        cols = columns(names, lengths, seqs, samples, mp["min_baseq"], bed=bed, flag_filter=mp["flag_filter"], min_mapq=mp["min_mapq"])
        tid_of = {n: i for i, n in enumerate(names)}
        keys = [(tid_of[ln.split("\t")[0]], int(ln.split("\t")[1]) - 1) for ln in text.split("\n")[:-1]]
        assert keys == sorted(cols), (case, set(keys) ^ set(cols))
        full = add_columns(text, names, cols, True, True)            # asserts every cell's count and quality string
        back, taken = strip_columns(full, 2)
        assert back == text
        for _, _, cnt, quals, (mq, bp) in taken:
            assert len(mq) == len(quals) and (bp == "*" if cnt == 0 else len(bp.split(",")) == cnt)
        have = {k[0] for k in keys}
        assert pushed_tids(names, seqs, samples, bed=bed, flag_filter=mp["flag_filter"], min_mapq=mp["min_mapq"]) == have, case
        n_lines += len(keys)
    assert n_lines > 20000


def test_fill_all_on_a_literal():
    names, lengths, seqs = ["c", "d", "e"], [8, 3, 2], ["ACGTACGT", "AC", None]
    text = "c\t3\tG\t1\t^].\t?\nc\t4\tT\t1\t.$\t?\nc\t9\tN\t1\t.\t?\n"                 # (position 9: a read over the contig's end keeps its line)
    z = "\t0\t*\t*"
    a = "".join("c\t%d\t%s%s\n" % (p, "ACGTACGT"[p - 1], z) for p in (1, 2)) + text[:text.index("c\t9")] + \
        "".join("c\t%d\t%s%s\n" % (p, "ACGTACGT"[p - 1], z) for p in (5, 6, 7, 8)) + "c\t9\tN\t1\t.\t?\n"
    assert fill_all(text, names, lengths, seqs, None, 1, 0, 0) == text
    assert fill_all(text, names, lengths, seqs, None, 1, 0, 1) == a
    assert fill_all(text, names, lengths, seqs, None, 1, 0, 2) == a + "d\t1\tA" + z + "\nd\t2\tC" + z + "\nd\t3\tN" + z + "\ne\t1\tN" + z + "\ne\t2\tN" + z + "\n"
    # a BED: the region of c cut inside, d absent, e whole; two samples and two extra columns on the filled lines
    two = "c\t3\tG\t1\t^].\t?\t]\t1\t0\t*\t*\t*\t*\n"
    z2 = "\t0\t*\t*\t*\t*" * 2
    bed = [(0, 1, 4), (2, 0, 50)]
    assert fill_all(two, names, lengths, seqs, bed, 2, 2, 1) == "c\t2\tC" + z2 + "\n" + two + "c\t4\tT" + z2 + "\n"
    assert fill_all(two, names, lengths, seqs, bed, 2, 2, 2) == "c\t2\tC" + z2 + "\n" + two + "c\t4\tT" + z2 + "\ne\t1\tN" + z2 + "\ne\t2\tN" + z2 + "\n"
    assert fill_all("", names, lengths, seqs, None, 1, 0, 1) == ""
