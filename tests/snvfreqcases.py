"""Tables for the SNV-frequency curves (tests/test_snvfreq_model.py, tests/test_gpu_snvfreq.py).

edge_table(n, S): the percent scale.  Every column cycles through EDGE_VALUES -- every integer 0..51 and 99, 100, the neighbouring doubles of each
on both sides, 49.5 and 50.5, 0.07 * 100 and 0.29 * 100 as doubles, NaN -- from its own starting point and with its own stride, so no two columns
agree once the table has two rows.  The two neighbours that leave [0, 100] (below 0, above 100) are not in it: the stage refuses them, and they
are OUTSIDE, for the refusal tests.  A column whose index is 5, 6 or 7 modulo 61 is constant 0.0, constant 100.0 or all NaN.  Column s does not
depend on S: a narrower table is the first columns of a wider one, so one model run serves every width.

random_unit_table(seed, n, S): [0, 1] rounded to 4 decimals as metaSNV_Filtering.py writes it, NaN holes (-1 in the file)."""
import functools

import numpy as np

import snvfreqmodel as model


def _edge_values():
    v = []
    for k in list(range(0, 52)) + [99, 100]:
        x = float(k)
        v += [y for y in (np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)) if 0.0 <= y <= 100.0]
    v += [49.5, 50.5, 0.07 * 100, 0.29 * 100, float("nan")]
    return np.array(v, dtype=np.float64)


EDGE_VALUES = _edge_values()
OUTSIDE = (float(np.nextafter(0.0, -np.inf)), float(np.nextafter(100.0, np.inf)), -0.5, 100.5, float("inf"), float("-inf"))
STRIDES = (1, 2, 4, 7, 8, 13)                              # coprime to len(EDGE_VALUES) = 165 = 3 * 5 * 11
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 513)
BANDS = ((10.0, 90.0), (7.000000000000001, 93.0), (43.99999999999999, 56.00000000000001))
CONSTANT = {5: 0.0, 6: 100.0, 7: float("nan")}              # column index modulo 61


def edge_table(n, S):
    L = EDGE_VALUES.size
    assert L == 165 and S <= L * len(STRIDES)
    p, s = np.arange(n, dtype=np.int64)[:, None], np.arange(S, dtype=np.int64)[None, :]
    stride = np.array(STRIDES, dtype=np.int64)[s // L]
    t = EDGE_VALUES[(p * stride + s) % L]
    for r, v in CONSTANT.items():
        t[:, r::61] = v
    return np.ascontiguousarray(t)


@functools.lru_cache(maxsize=None)
def edge_counts(n, band=BANDS[0]):
    """The model's counts of the widest edge table of n rows; a table of S columns has the first S rows of each array.  Read-only."""
    c = model.counts(edge_table(n, max(WIDTHS)), band[0], band[1])
    for a in c.values():
        a.setflags(write=False)
    return c


def random_unit_table(seed, n, S, uncovered_columns=()):
    """Column s leans to the ends of [0, 1] with its own probability, so the shares of fixed positions spread over (0, 1) across the samples."""
    rng = np.random.default_rng(seed)
    lean = rng.random(S)
    flat = rng.random((n, S))
    end = np.where(rng.random((n, S)) < 0.5, rng.random((n, S)) * 0.08, 1.0 - rng.random((n, S)) * 0.08)
    t = np.round(np.where(rng.random((n, S)) < lean[None, :], end, flat), 4)
    t[rng.random((n, S)) < 0.15] = np.nan
    for s in uncovered_columns:
        t[:, s] = np.nan
    return t


def sample_names(S):
    return ["s%04d.bam" % (i + 1) for i in range(S)]


def write_freq(path, names, table):
    """<species>.filtered.freq: positions x samples on the [0, 1] scale, -1 where a sample has no coverage (NaN here)."""
    with open(path, "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        for p, row in enumerate(table):
            f.write("c1:-:%d:A:." % (p + 1) + "\t" + "\t".join("-1" if v != v else repr(float(v)) for v in row) + "\n")


STAGE_SHAPE = (1100, 37)                                    # rows x samples of the file-stage table; its last sample has no covered cell
STAGE_OPTS = ({}, {"max_prop_reads_non_homog": 0.07, "min_prop_homog_snv": 0.5}, {"max_prop_reads_non_homog": 0.29})


@functools.lru_cache(maxsize=None)
def stage_table():
    t = random_unit_table(20241, STAGE_SHAPE[0], STAGE_SHAPE[1], uncovered_columns=(STAGE_SHAPE[1] - 1,))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def stage_files(opts_index):
    """(files, result) of the model for the stage table at STAGE_OPTS[opts_index]; the cells are multiplied by 100 in double as the stage does."""
    return model.files(sample_names(STAGE_SHAPE[1]), stage_table() * 100.0, "sp", **STAGE_OPTS[opts_index])
