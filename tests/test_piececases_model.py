"""The seam cases of the device per-read stage (tests/piececases.py) hold what they claim, and the reference side of every GPU check on
them (tests/test_gpu_piece_seams.py) is pinned without a GPU: a closed-form model of the quality edits and of the -Q test, written here,
gives the oracle's calls on families A and D at every cutoff of CUTOFFS_ORACLE; the host stage's edited qualities give the oracle's mpileup
text on family D; the ten further IUPAC codes of family C2 make the oracle report its domain error (why C2 is device against host only).

The model.  Overlapping mates (sam.c tweak_overlap_quality [EXT]), for every reference position where both mates of a pair hold a base:
  agreeing bases:     the first mate gets min(200, x + y), the other 0;
  disagreeing bases:  int(0.8 * max(x, y)) goes to the higher quality (ties: the first mate), 0 to the other.
A base is counted iff its edited quality is at least Q -- so at -Q 0 the zeroed mate is counted too.  Only A, C, G, T count (a read without
SEQ shows N).  snpCall drops the first line of the text."""
import numpy as np
import pytest

import bamtools as bt
import orc
import piececases as pc
from metasnv_amd import core

SC = dict(min_coverage=1, calling_threshold=1, calling_min_fraction=0.0)


def _aligned(r):
    """(reference position, index of the base in the read) of every aligned base of a decoded record."""
    rp, q, out = r["pos"], 0, []
    for l, op in r["cigar"]:
        if op in (0, 7, 8):
            out += [(rp + i, q + i) for i in range(l)]
            rp += l; q += l
        elif op in (2, 3):
            rp += l
        elif op in (1, 4):
            q += l
    return out


def _records(stream):
    """bamtools.iter_records plus the mate position (which decides whether an alignment waits for its mate)."""
    import struct
    recs = list(bt.iter_records(stream))
    for r, (off, _, _, _) in zip(recs, pc.record_offsets(stream)):
        r["mpos"] = struct.unpack_from("<i", bytes(stream[off + 28:off + 32]))[0]
    return recs


def model_edit(recs):
    """The qualities the pileup sees: the rule of the module docstring over the alignments of one sample in file order.  An alignment of a
    proper pair finds the waiting alignment of its name (which then leaves, edited if the two overlap) or waits itself."""
    quals = [list(r["qual"]) for r in recs]
    waiting = {}
    for i, r in enumerate(recs):
        if not r["flag"] & 2:
            continue
        j = waiting.pop(r["name"], None)
        if j is not None:
            a, b = recs[j], r
            if a["seq"] and b["seq"]:
                at_b = dict(_aligned(b))
                for p, qa in _aligned(a):
                    if p not in at_b:
                        continue
                    qb = at_b[p]
                    x, y = quals[j][qa], quals[i][qb]
                    if a["seq"][qa] == b["seq"][qb]:
                        quals[j][qa], quals[i][qb] = min(200, x + y), 0
                    elif x >= y:
                        quals[j][qa], quals[i][qb] = int(0.8 * x), 0
                    else:
                        quals[j][qa], quals[i][qb] = 0, int(0.8 * y)
                continue
        if r["mpos"] >= r["pos"]:
            waiting[r["name"]] = i
    return quals


def model_calls(case, cutoff, edit=model_edit):
    """called_SNPs text of a case at min_coverage = 1, calling_threshold = 1, min_fraction = 0."""
    names, lengths, seqs, samples = case
    S, counts, first = len(samples), {}, None
    for s, smp in enumerate(samples):
        recs = _records(smp)
        for r, q in zip(recs, edit(recs)):
            for p, k in _aligned(r):
                first = p if first is None or p < first else first
                b = r["seq"][k] if r["seq"] else "N"
                if b in "ACGT" and q[k] >= cutoff and p < lengths[0]:
                    counts.setdefault(p, {}).setdefault(b, [0] * S)[s] += 1
    lines = []
    for p in sorted(counts):
        ref = seqs[0][p].upper() if p < len(seqs[0]) else "N"
        alleles = [(b, c) for b, c in ((b, counts[p].get(b)) for b in "ACTG") if c and b != ref]
        if p == first or not alleles:
            continue
        cov = [sum(c[s] for c in counts[p].values()) for s in range(S)]
        lines.append("%s\t-\t%d\t%s\t%s\t%s" % (names[0], p + 1, ref, "|".join(map(str, cov)), ",".join("%d|%s|.|%s" % (sum(c), b, "|".join(map(str, c))) for b, c in alleles)))
    return "".join(l + "\n" for l in lines)


@pytest.fixture(scope="module")
def cases():
    return dict(a=pc.family_a(), b=pc.family_b(), c1=pc.family_c(), c2=pc.family_c(bt.NT16), d=pc.family_d(), e=pc.family_e())


# ---------------------------------------------------------------------------------- the cases hold what they claim
def test_family_a_puts_every_quality_in_every_byte_slot_and_lane(cases):
    a = cases["a"]
    for reads in a.meta["reads"]:
        seen = {(q[j], j % 8) for _, q in reads for j in range(len(q))}
        lanes = {(q[j], j // 32) for _, q in reads for j in range(len(q))}
        for v in pc.Q_FLAG:
            assert all((v, slot) in seen for slot in range(8)), v
            assert all((v, lane) in lanes for lane in range(4)), v
        assert sum(1 for _, q in reads if set(q) == {255}) == len(reads) // 8 == sum(1 for _, q in reads if set(q) == {0})
    # the SEQ and the QUAL fields start at every residue mod 4 -- in the stream and, with it, in a window that starts on 16 bytes
    for smp in a[3]:
        offs = pc.record_offsets(smp)
        assert {o[1] % 4 for o in offs} == {0, 1, 2, 3} and {o[2] % 4 for o in offs} == {0, 1, 2, 3}
    last = pc.record_offsets(a[3][-1])[-1]
    assert last[2] + a.meta["read_len"] == last[0] + last[3]            # no aux bytes behind the round's last qualities


def test_every_seam_sample_fits_the_image_form_of_the_emit_kernel(cases):
    for key, case in cases.items():
        for smp in case[3]:
            offs = pc.record_offsets(smp)
            assert len(offs) % pc.PB == 0 and len(offs) > 0, key
            for b in range(0, len(offs), pc.PB):
                assert offs[b + pc.PB - 1][0] + offs[b + pc.PB - 1][3] - (offs[b][0] & ~15) <= pc.EW_BYTES, (key, b)
        # no record opens with the <l_seq>S placeholder of a CIGAR kept in the CG field
        for smp in case[3]:
            for r in bt.iter_records(smp):
                assert not (r["cigar"] and r["cigar"][0] == (len(r["seq"]), 4)), key
    for key in ("a", "b", "c1", "c2"):                                # pieces per block: the seq stretch and the further pieces (a record's first piece has its own slot)
        for smp in cases[key][3]:
            recs = list(bt.iter_records(smp))
            for b in range(0, len(recs), pc.PB):
                blk = bt.records(*[bt.make_record(0, r["pos"], "".join("%d%s" % (n, bt.CIGAR_OPS[op]) for n, op in r["cigar"]), r["seq"], qual=r["qual"]) for r in recs[b:b + pc.PB]])
                pcs = pc.pieces(blk)
                assert len(pcs) - pc.PB <= pc.EQ_CAP, (key, b)
                assert sum((n + 3) // 4 * 2 for _, n in pcs) + 16 <= pc.EO_BYTES, (key, b)


def test_family_b_holds_every_piece_length_and_every_tile_edge_distance(cases):
    b = cases["b"]
    recs = list(bt.iter_records(b[3][0]))
    for n in pc.PIECE_LEN:
        for clip in (0, 1):
            want = ([(1, 4)] if clip else []) + [(n, 0)]
            assert any(r["cigar"] == want for r in recs), (n, clip)
    assert sorted(b.meta["lens"]) == sorted((n, c) for n in pc.PIECE_LEN for c in (0, 1))
    pcs = pc.pieces(b[3][0])
    assert len(pcs) == b.meta["n_pieces"]
    for d in pc.EDGE_BEFORE:                                          # the read is cut at the edge: d bases in front, 40 - d behind
        assert any(n == d and (g + n) % pc.TILE == 0 for g, n in pcs) and any(n == 40 - d and g % pc.TILE == 0 for g, n in pcs), d
    pads = {(min(3, pc.TILE - (g + n) % pc.TILE), n % 4) for g, n in pcs if (g + n) % pc.TILE and pc.TILE - (g + n) % pc.TILE <= 4}
    assert {p for p, _ in pads} == {1, 2, 3} and any((g + n) % pc.TILE == 0 for g, n in pcs)      # pad_in_tile 0 .. 3
    assert {(p, m) for p, m in pads if m} >= {(1, 1), (1, 3), (2, 1), (2, 2), (3, 1), (3, 3)}     # n_pad = min(4 - n % 4, pad_in_tile): 1, 2 and 3
    assert {n for _, n in pcs} >= {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128}
    assert any(r["tid"] == 0 and r["pos"] < b[1][0] < r["pos"] + 40 for r in recs)                          # over the contig's end
    assert len(b[2][1]) < b[1][1] and any(r["tid"] == 1 and r["pos"] < len(b[2][1]) < r["pos"] + 40 <= b[1][1] for r in recs)      # over the FASTA record's end, inside the contig
    for r in recs:                                                    # 13, 12 alternating: every base's flag differs from its neighbour's at -Q 13
        q = r["qual"][1:] if r["cigar"][0][1] == 4 else r["qual"]
        assert all((x >= 13) != (y >= 13) for x, y in zip(q, q[1:])) and set(q) <= {12, 13}


def test_family_c_runs_every_code_through_every_nibble_slot_over_every_reference_letter(cases):
    for key, codes in (("c1", pc.BASES_ORACLE), ("c2", bt.NT16)):
        c = cases[key]
        ref = c[2][0]
        slots, over = set(), set()
        for r in bt.iter_records(c[3][0]):
            clip = r["cigar"][0][0] if r["cigar"][0][1] == 4 else 0
            for p, k in _aligned(r):
                slots.add((r["seq"][k], (k - clip) % 32, clip & 1))
                over.add((r["seq"][k], ref[p]))
        for b in codes:
            assert all((b, slot, par) in slots for slot in range(32) for par in (0, 1)), b
            assert all((b, x) in over for x in "ACGTNacgtn"), b
        assert c.meta["n_pieces"] >= 48 and len(c.meta["sampled"]) >= 3
        assert any(n < 16 for n in c.meta["sampled"]) and any(17 <= n <= 31 for n in c.meta["sampled"])


def test_family_d_holds_every_pair_of_qualities_for_both_kinds(cases):
    d = cases["d"]
    recs = _records(d[3][0])
    by_pos = {}
    for r in recs:
        if r["flag"] & 2 and r["cigar"] == [(23, 0)]:
            by_pos.setdefault(r["pos"], []).append(r)
    seen = {"agree": set(), "differ": set()}
    for p, rr in by_pos.items():
        if len(rr) == 2 and rr[0]["name"] == rr[1]["name"]:
            kind = "agree" if rr[0]["seq"] == rr[1]["seq"] else "differ"
            seen[kind] |= set(zip(rr[0]["qual"], rr[1]["qual"]))
    want = {(x, y) for x in pc.Q_OVL for y in pc.Q_OVL}
    assert seen["agree"] == want and seen["differ"] == want
    for kind in ("agree", "differ"):
        p = pc.d_position(d, kind, 128, 255)
        assert [r["qual"][p - r["pos"]] for r in by_pos[p - pc.Q_OVL.index(255)]] == [128, 255]
    assert sum(1 for r in recs if (10, 0) in r["cigar"] and (2, 2) in r["cigar"]) == 2 * len(pc.Q_OVL)
    r1 = _records(d[3][1])
    assert sum(1 for r in r1 if r["name"] == "tmpl") == pc.OVL_SLOTS
    assert any(r["flag"] & 2 and not r["seq"] for r in r1) and sum(1 for r in r1 if set(r["qual"]) == {255}) == 2
    for smp in d[3]:                                                  # file order is sorted
        pos = [r["pos"] for r in bt.iter_records(smp)]
        assert pos == sorted(pos)


def test_family_e_shares_its_reads_and_stacks_past_the_token(cases):
    e = cases["e"]
    r0, r1 = list(bt.iter_records(e[3][0])), list(bt.iter_records(e[3][1]))
    assert [r for r in r1 if r["name"].startswith("e")] == r0
    stack = [r for r in r1 if r["pos"] == e.meta["stack_pos"]]
    assert 3 * len(stack) > e.meta["token_limit"] > len(stack) + 2 * len(r0[0]["seq"])      # cut where the reads start (3 characters each), nowhere else
    assert {q for r in r0 for q in r["qual"]} == set(pc.E_QUALS) == {q for r in stack for q in r["qual"]}
    assert not any(r["pos"] <= e.meta["stack_pos"] < r["pos"] + 20 for r in r0)


# ---------------------------------------------------------------------------------- the reference is pinned
@pytest.mark.parametrize("cutoff", pc.CUTOFFS_ORACLE)
@pytest.mark.parametrize("key", ["a", "d"])
def test_the_closed_form_model_gives_the_oracle_calls(cases, key, cutoff):
    names, lengths, seqs, samples = cases[key]
    got = orc.call(names, lengths, seqs, samples, mp=dict(min_baseq=cutoff), sc=SC)
    want = model_calls(cases[key], cutoff)
    assert got[0] == want
    assert want.count("\n") > 1000
    if key == "d":                                                    # the named positions of the GPU test, from the model
        at = pc.calls_at(want)
        p = lambda kind, x, y: at.get(pc.d_position(cases[key], kind, x, y), ([0, 0], {}))[0][0]
        if cutoff == 13:
            assert p("agree", 128, 128) == 1 and p("agree", 255, 255) == 1        # (a sum taken in 8 bits: 0 and 254 -- the first would not be counted)
            assert p("differ", 16, 0) == 0 and p("differ", 17, 0) == 1           # 0.8 x 16 truncates to 12, 0.8 x 17 to 13
        if cutoff == 0:
            assert p("agree", 1, 1) == 2                                          # the zeroed mate is counted at -Q 0


def test_family_a_shows_each_flag_in_the_oracle_text(cases):
    """One position per quality byte: the count at the position is the byte's flag."""
    a = cases["a"]
    for cutoff in pc.CUTOFFS_ORACLE:
        at = pc.calls_at(orc.call(*a, mp=dict(min_baseq=cutoff), sc=SC)[0])
        for s, reads in enumerate(a.meta["reads"]):
            for pos, q in reads[1:]:
                for j in (0, 1, 7, 8, 31, 32, 63, 64, 95, 96, 126, 127):
                    assert (at.get(pos + j, ([0, 0], {}))[0][s] == 1) == (q[j] >= cutoff), (cutoff, s, pos, j, q[j])


def test_host_stage_edits_family_d_like_the_oracle(cases):
    names, lengths, seqs, samples = cases["d"]
    n_edited = 0
    for smp in samples:
        ds = core.Dataset(None, names, lengths, seqs)
        edited = ds.pileup_qualities(smp)
        ds.close()
        n_edited += int((edited != smp).sum())
        want = orc.mpileup_text(names, lengths, seqs, [smp], mp=dict(min_baseq=0))
        got = orc.mpileup_text(names, lengths, seqs, [edited], mp=dict(min_baseq=0, ignore_overlaps=1))
        assert got == want
        assert orc.mpileup_text(names, lengths, seqs, [smp], mp=dict(min_baseq=0, ignore_overlaps=1)) != want
        quals = [q for r, q in zip(_records(smp), model_edit(_records(smp)))]
        assert [r["qual"] for r in bt.iter_records(edited)] == quals          # ... and like the model, byte for byte
    assert n_edited > 3000
    edited = set(int(q) for r in bt.iter_records(_host_edit(cases["d"], 0)) for q in r["qual"])
    assert {200, 204, 12, 13, 63, 64, 126, 127} <= edited           # the cap, int(0.8 x 255), and both sides of every cutoff behind the truncation


def _host_edit(case, s, **kw):
    names, lengths, seqs, samples = case
    ds = core.Dataset(None, names, lengths, seqs, core.default_params(**kw) if kw else None)
    try:
        return ds.pileup_qualities(samples[s])
    finally:
        ds.close()


@pytest.mark.parametrize("cutoff", [0, 13])
def test_family_e_is_cut_behind_the_hundredth_read_of_the_stack(cases, cutoff):
    """The oracle with a token of token_limit characters counts the stack's first 100 reads where they start (`^`, mapq, base: read r's base
    is character 3 r + 2) and every read everywhere else, stored bytes of 128 and more included; the host stage marks the other 28 bases
    (quality 0 at this seam) and clamps every other quality of that sample to 127, and leaves the shallow sample alone."""
    e = cases["e"]
    T, p0, n_stack = e.meta["token_limit"], e.meta["stack_pos"], len(e.meta["stack_quals"])
    at = pc.calls_at(orc.call(*e, mp=dict(min_baseq=cutoff), sc=dict(SC, token_cap=T))[0])
    assert at[p0][0] == [0, T // 3] and all(at[p0 + j][0] == [0, n_stack] for j in range(1, e.meta["stack_len"]))
    assert all(at[pos + j][0] == [1, 1] for pos, q in e.meta["shared"][1:] for j in range(len(q)))
    same, cut = _host_edit(e, 0, min_baseq=cutoff, token_limit=T), _host_edit(e, 1, min_baseq=cutoff, token_limit=T)
    assert np.array_equal(same, e[3][0])
    changed = cut != e[3][1]
    assert int((cut[changed] == 0).sum()) == n_stack - T // 3 and set(cut[changed].tolist()) == {0, 127}
    assert max(max(r["qual"]) for r in bt.iter_records(cut)) == 127


def test_the_further_iupac_codes_are_outside_the_oracle_domain(cases):
    """The reference snpCall dereferences an empty vector at a base code other than = A C G T N; the oracle reports that as a domain error.
    Family C2 is therefore checked device against host only."""
    with pytest.raises(orc.OrcError) as e:
        orc.call(*cases["c2"], mp=dict(min_baseq=13), sc=SC)
    assert e.value.code == orc.ERR_DOMAIN
    assert orc.call(*cases["c1"], mp=dict(min_baseq=13), sc=SC)[0].count("\n") > 100
