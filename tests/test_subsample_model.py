"""The read subsampler's rule (`qaCompute -a`): the plain-Python model (tests/subsamplemodel.py) against the issue's known answers, and the
library's host entries -- msnv_subsample_seed_word, msnv_subsample_keep, msnv_records_subsample -- against the model.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

import bamtools as bt
import subsamplemodel as sm
from metasnv_amd import _lib, core

# name, seed, x31 (None: not stated), k, k & 0xffffff (None: not stated)
KNOWN = [(b"r0", 0, 0xdfe, 0x154b4874, 4933748),
         (b"r0", 42, None, 0xca004ac5, 19141),
         (b"read/1", 0, 0xc84551f8, 0xec530e6b, None),
         (b"read/1", 42, None, 0x2de795c2, None),
         (b"A", 0, None, 0xfffceb8d, None),
         (b"", 0, 0, 0x4636b9c9, None),
         (b"q\xe9", 0, 0xd98, 0xf8b8cca7, None)]
KEPT = {(0, .5): (34, 125, 2053), (42, .25): (17, 64, 1041), (7, .9): (55, 235, 3685), (42, 1e-7): (0, 0, 0)}
FRACS = (1e-7, .25, .5, .9, 1 - 2.0 ** -24, 1.0, 2.0)


def _keep_lib(name, word, frac):
    return bool(_lib.lib.msnv_subsample_keep(name, word, frac))


def test_the_model_gives_the_known_answers():
    assert [sm.seed_word(s) for s in (0, 1, 42, 7)] == [0, 1804289383, 71876166, 1045618677]
    for name, seed, x, k, low in KNOWN:
        if x is not None:
            assert sm.x31(name) == x, name
        assert sm.mixed(name, sm.seed_word(seed)) == k, (name, seed)
        if low is not None:
            assert k & 0xffffff == low
    for (seed, frac), counts in KEPT.items():
        w = sm.seed_word(seed)
        for n, want in zip((64, 257, 4096), counts):
            assert sum(sm.keep(b"r%d" % i, w, frac) for i in range(n)) == want, (seed, frac, n)


def test_the_seed_word_is_libcs_and_bad_seeds_are_refused():
    for seed in (0, 1, 42, 7, 123456789, 0xffffffff):
        assert core.subsample_seed_word(seed) == sm.seed_word(seed), seed
    assert core.subsample_seed_word(1) == 1804289383
    for bad in (-1, -3, 1 << 32, (1 << 32) + 5):
        with pytest.raises(_lib.MsnvError) as e:
            core.subsample_seed_word(bad)
        assert e.value.code == _lib.EINVAL


def test_keep_equals_the_model_on_known_and_random_names():
    rnd = random.Random(20261021)
    names = [k[0] for k in KNOWN] + [b"r%d" % i for i in range(300)]
    for _ in range(3000):
        n = rnd.choice([0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 254, rnd.randrange(0, 255)])
        hi = rnd.random() < 0.4                                  # bytes of 0x80 and more among them (signed chars), never a NUL
        names.append(bytes(rnd.randrange(128, 256) if hi and rnd.random() < 0.5 else rnd.randrange(1, 128) for _ in range(n)))
    words = [sm.seed_word(s) for s in (0, 42, 7)]
    for name in names:
        for w in words:
            for frac in FRACS:
                # the library compares integers (threshold = ceil(frac * 2^24)); the model divides, as the reference does
                assert _keep_lib(name, w, frac) == sm.keep(name, w, frac), (name, w, frac)
    for name, seed, _, k, _ in KNOWN:                            # ... and the known words themselves, through the threshold just above and at them
        low, w = k & 0xffffff, sm.seed_word(seed)
        assert _keep_lib(name, w, (low + 1) / 2.0 ** 24) and not _keep_lib(name, w, low / 2.0 ** 24)


def _stream(n, rnd):
    """n records named r0 .. r{n-1} of several shapes, a few renamed to names with high bytes / no bytes."""
    recs = []
    for i in range(n):
        shape = i % 4
        name = "r%d" % i
        if shape == 0:
            r = bt.make_record(0, 10 + i, "*", "*", name=name, flag=4)
        elif shape == 1:
            r = bt.make_record(0, 10 + i, "7M", "ACGTACG", name=name, mtid=1, mpos=5 + i, tlen=40)
        elif shape == 2:
            r = bt.make_record(1, 10 + i, "3M1I3M", "ACGTACG", name=name, aux=bt.aux_fields(nm=1, md="6", score=-3))
        else:
            r = bt.make_record(1, 10 + i, "5M", "ACGTA", name=name, flag=1024)
        recs.append(r)
    return recs


def test_the_host_stream_form_returns_the_models_bytes_and_counts():
    rnd = random.Random(5)
    for n in (0, 1, 64, 257):
        recs = _stream(n, rnd)
        stream = b"".join(recs)
        for (seed, frac), counts in KEPT.items():
            want, kept, dropped = sm.filter_stream(stream, sm.seed_word(seed), frac)
            got, cn = core.subsample_records_host(np.frombuffer(stream, np.uint8), seed, frac)
            assert got == want and cn == (kept, dropped), (n, seed, frac)
            if n in (64, 257):
                assert kept == counts[(64, 257).index(n)]
        got, cn = core.subsample_records_host(np.frombuffer(stream, np.uint8), 42, 1.0)      # everything kept
        assert got == stream and cn == (n, 0)
        got, cn = core.subsample_records_host(np.frombuffer(stream, np.uint8), 42, 0.0)      # no subsampling: nothing is even counted
        assert got == stream and cn == (0, 0)
    # names with bytes >= 0x80, an empty name, a name of 254 bytes; mates share a fate
    odd = [b"", b"\xff", b"q\xe9", bytes(range(1, 255)), b"\x80" * 33]
    recs = []
    for k, nm in enumerate(odd * 6):
        r = bt.make_record(0, k, "4M", "ACGT", name="x" * len(nm), mtid=0, mpos=k + 50)
        recs.append(sm.with_name(r, nm))
    stream = b"".join(recs)
    for seed, frac in ((0, .5), (42, .25), (7, .9)):
        want, kept, dropped = sm.filter_stream(stream, sm.seed_word(seed), frac)
        got, cn = core.subsample_records_host(np.frombuffer(stream, np.uint8), seed, frac)
        assert got == want and cn == (kept, dropped) and kept % 6 == 0
    # a chain that breaks is MSNV_EFORMAT
    with pytest.raises(_lib.MsnvError) as e:
        core.subsample_records_host(np.frombuffer(stream[:-3], np.uint8), 42, .25)
    assert e.value.code == _lib.EFORMAT


def test_the_argument_is_read_like_qacomputes():
    for text, want in (("42.25", (42, .25)), ("0.5", (0, .5)), (".5", (0, .5)), ("7.9", (7, .9)), ("1", (1, 0.0))):
        assert sm.parse_arg(text) == want and core.parse_subsample(text) == want, text
    for text in ("-3.5", "4294967296.5"):
        with pytest.raises(ValueError):
            sm.parse_arg(text)
        with pytest.raises(ValueError):
            core.parse_subsample(text)


def test_a_dataset_takes_the_setting_only_before_its_first_sample():
    """Host-only dataset (no context): the setting, the host route's filter and the refusal once a sample is in."""
    rnd = random.Random(9)
    stream = np.frombuffer(b"".join(bt.make_record(0, 10 + i, "7M", "ACGTACG", name="r%d" % i) for i in range(257)), np.uint8)
    ds = core.Dataset(None, ["c0", "c1"], [5000, 5000])
    ds.set_subsample(42, .25)
    assert ds.subsample == (42, .25)
    ds.add_sample_records(stream)
    assert int(ds.sample_stats(0)[core.STATS_FIELDS.index("total_reads")]) == 64
    with pytest.raises(_lib.MsnvError) as e:
        ds.set_subsample(7, .5)
    assert e.value.code == _lib.EINVAL
    ds.close()
    ds = core.Dataset(None, ["c0", "c1"], [5000, 5000])
    ds.set_subsample(42, 0.0)                                   # off
    assert ds.subsample is None
    ds.add_sample_records(stream)
    assert int(ds.sample_stats(0)[core.STATS_FIELDS.index("total_reads")]) == 257
    ds.close()
