"""Inputs shared by tests/test_profile_model.py and tests/test_gpu_profile.py: matrices of genotyping SNV frequencies in the cell mixes the kernel
has to cope with, and the files of the stage with planted subspecies."""
import numpy as np

from genotypecases import sample_names

MIXES = ("real", "equal", "low_bits", "nan_column", "one_called", "two_called", "neg_zero")


def matrix(mix, g, s, seed):
    """[g x s] in [0, 100] with NaN.  real: about 45 % exact 0, 45 % exact 100, the rest distinct, NaN scattered (n differs per column); equal: one
    value everywhere; low_bits: 50 + i * 2^-44, distinct cells that differ only in low mantissa bits (no pass of a radix selection may be skipped);
    nan_column / one_called / two_called: the last column holds no, one, two called cells; neg_zero: -0.0 among the zeros."""
    rng = np.random.default_rng([seed, g, s])
    u = rng.uniform(size=(g, s))
    real = np.where(u < 0.45, 0.0, np.where(u < 0.9, 100.0, rng.uniform(0, 100, size=(g, s))))
    real[rng.uniform(size=(g, s)) < 0.1] = np.nan
    if mix == "real":
        return real
    if mix == "equal":
        return np.full((g, s), 37.5)
    if mix == "low_bits":
        return 50.0 + rng.permutation(g * s).reshape(g, s) * 2.0 ** -44
    if mix == "neg_zero":
        real[real == 0.0] = np.where(rng.uniform(size=int((real == 0.0).sum())) < 0.5, -0.0, 0.0)
        return real
    real[:, -1] = np.nan
    if mix in ("one_called", "two_called"):
        real[g // 2, -1] = 12.25
    if mix == "two_called" and g > 1:
        real[0, -1] = 100.0
    return real


def flips(g, seed, share=0.5):
    return np.random.default_rng([seed, g]).uniform(size=g) < share


# ---------------------------------------------------------------------------------------------- the stage
def freq_text(ids, rows):
    """<species>_<cluster>.pos.freq as convertSNVtoAlleleFreq.py writes it: id, then str(float) per sample, -1 for no coverage."""
    return "".join(i + "\t" + "\t".join("-1" if v != v else repr(float(v)) for v in r) + "\n" for i, r in zip(ids, rows))


def hap_text(pos_ids, flip):
    """<species>_<cluster>_hap_positions.tab as writeGenotypeFreqs.py writes it."""
    return "posId\tflip\n" + "".join("%d\t%s\t%s\n" % (k + 1, p, "TRUE" if f else "FALSE") for k, (p, f) in enumerate(zip(pos_ids, flip)))


def all_samples_text(names):
    return "".join("/data/run1/bams/%s\n" % n for n in names)


LOW_COVERAGE, SUM_HIGH, SUM_LOW, BAD, MIXED = 5, 6, 7, 8, 9             # the samples of planted_project that are not plain


def planted_project(species="sp", n_samples=40, sizes=(30, 45, 60), seed=11):
    """Three clusters with 30, 45 and 60 genotyping positions.  Sample s carries subspecies s % 3 + 1: near 100 at its cluster's positions (near 0 in the
    file where the position is flipped), near 0 at the others'.  Sample 5 has coverage at a tenth of the positions (dropped from every cluster), 6
    carries subspecies 1 and 2 at once (sums to about 200), 7 none (sums to 0), 8 its own with 40 % of the positions at exact 0 (median 100, prevalence
    0.6: bad), 9 a 60 / 40 mix of 1 and 2 (coherent, assigned to none).  One listed position of cluster 2 is absent from its .pos.freq; every
    .pos.freq holds rows of other alleles that no positions file lists.  Returns (tree: name -> text, all_samples text, truth [n_samples])."""
    rng = np.random.default_rng(seed)
    names = sample_names(n_samples)
    truth = np.arange(n_samples) % 3 + 1
    tree = {}
    for c, g in enumerate(sizes, start=1):
        flip = rng.uniform(size=g) < 0.4
        share = np.where(truth == c, 1.0, 0.0)
        share[SUM_HIGH] = 1.0 if c in (1, 2) else 0.0
        share[SUM_LOW] = 0.0
        share[MIXED] = {1: 0.6, 2: 0.4}.get(c, 0.0)
        noise = np.where(rng.uniform(size=(g, n_samples)) < 0.7, 0.0, rng.uniform(0, 6, size=(g, n_samples)).round(2))
        data = np.abs(share[None, :] * 100.0 - noise)                  # as the statistics see it
        if truth[BAD] == c:
            data[rng.permutation(g)[:int(0.4 * g)], BAD] = 0.0
        data[rng.uniform(size=(g, n_samples)) < 0.05] = np.nan
        data[rng.permutation(g)[:g - g // 10], LOW_COVERAGE] = np.nan
        rows = np.where(flip[:, None], 100.0 - data, data)              # as the file holds it
        pos = 1000 * c + np.arange(g)
        ids = ["ctg.%d:%s:%d:A" % (c, "-" if p % 2 else "gene%d" % p, p) for p in pos]
        pos_ids = ["ctg.%d:%s:%d:T>A:%s" % (c, "-" if p % 2 else "gene%d" % p, p, "." if p % 2 else "N[AAT-ACT]") for p in pos]
        others = ["ctg.%d:-:%d:C" % (c, p) for p in pos[::7]]
        order = rng.permutation(g + len(others))                       # the .pos.freq is in the order of the SNV calls, not of the positions file
        all_ids = ids + others
        all_rows = np.concatenate([rows, rng.uniform(0, 100, size=(len(others), n_samples)).round(3)])
        keep = [k for k in order if not (c == 2 and k == 3)]           # cluster 2's position 3 is absent
        tree["%s_%d.pos.freq" % (species, c)] = freq_text([all_ids[k] for k in keep], all_rows[keep])
        tree["%s_%d_hap_positions.tab" % (species, c)] = hap_text(pos_ids, flip)
    return tree, all_samples_text(names), truth
