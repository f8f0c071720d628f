"""The host DEFLATE decoder (metasnv_amd/csrc/inflate.cpp, and zlib behind it in hostio.cpp) on the hand-assembled streams of
tests/deflate_craft.py: constructs no compressor writes (15-bit codes with the deepest subtables, distance codes behind the root table,
code-length repeats across the two tables, every length and distance symbol, overlapping copies at every small distance, stored blocks
behind every bit offset) and every malformed construct on its own.  The judge is zlib: what it accepts the decoders must decode to the
same bytes, what it refuses they must refuse -- a file htslib cannot read is not read here either."""
import ctypes as C
import os
import subprocess

import pytest

import deflate_craft as dc
from metasnv_amd import core, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["code_shapes", "max_tables", "code_length_stream", "every_symbol", "overlap", "window", "literal_batching", "stored", "stored_seam",
            "several_blocks", "malformed"]


def test_writer_against_zlib():
    """zlib's verdict on every case is the intended one: the bytes of expand(tokens) for a valid case, an error (or a stream that does not
    end, or another size than ISIZE) for a malformed one.  Case() asserts that while the corpus is generated; here again, case by case."""
    cases = dc.corpus()
    assert sorted({c.family for c in cases}) == sorted(FAMILIES)
    for c in cases:
        got = dc.judge(c.stream, len(c.intended))
        assert (got == c.intended) if c.valid else (got is None), c.name
    assert len(dc.valid_cases()) > 900 and len(dc.malformed_cases()) > 60
    # the cases the kernel's input window is pinned on: the file puts their payloads at all four byte alignments
    data, want = dc.valid_file()
    offs = dc.payload_offsets(data)
    cs = dc.valid_cases()
    assert len(offs) == len(cs) + 1
    for fam in ("window", "stored_seam"):
        assert {(c.align, o % 4) for c, o in zip(cs, offs) if c.family == fam} == {(a, a) for a in range(4)}
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    # the sets that need the most table entries fit zlib's bounds (the kernel's caps) and the host decoder's arrays
    for (key, seed), size in dc.MAX_TABLE_HISTS.items():
        assert size <= {"ll_root9": 852, "d_root6": 592, "ll_root11": 2048 + 1200, "d_root8": 256 + 600}[key]


def _has_bmi2():
    try:
        return " bmi2 " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def test_decoder_on_the_corpus_under_sanitizers(tmp_path):
    """inflate_raw (and inflate_raw_bmi2 where the build host has BMI2) built with -fsanitize=address,undefined: every valid case accepted
    with the right bytes, every malformed case refused, no sanitizer report (exact-size output buffers, 8 readable bytes behind the input)."""
    exe = str(tmp_path / "inflate_harness")
    csrc = os.path.join(ROOT, "metasnv_amd", "csrc")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = [os.path.join(ROOT, "tests", "native", "inflate_harness.cpp"), os.path.join(csrc, "inflate.cpp")]
    decoders = ["inflate_raw"]
    if _has_bmi2():
        obj = str(tmp_path / "inflate_bmi2.o")
        subprocess.check_call(flags + ["-mbmi2", "-c", os.path.join(csrc, "inflate_bmi2.cpp"), "-o", obj])
        src.append(obj); flags.append("-DMSNV_HARNESS_BMI2"); decoders.append("inflate_raw_bmi2")
    subprocess.check_call(flags + src + ["-lz", "-o", exe])
    cases = dc.corpus()
    path = str(tmp_path / "corpus.bin")
    open(path, "wb").write(dc.container(cases))
    r = subprocess.run([exe, "corpus", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "corpus: %d cases" % len(cases)
    got = {}
    for ln in lines[:-1]:
        dec, name, verdict, same = ln.split(" ")
        got[(dec, name)] = (verdict, same)
    assert len(got) == len(cases) * len(decoders)
    wrong = [(dec, c.name, got[(dec, c.name)]) for dec in decoders for c in cases
             if got[(dec, c.name)] != (("accepted", "match") if c.valid else ("refused", "-"))]
    assert not wrong, wrong[:20]


def _fallbacks():
    n = C.c_uint64()
    _lib.lib.msnv_host_stats(C.byref(n))
    return n.value


def test_host_decoder_through_the_library(tmp_path):
    """The corpus as BGZF files through bgzf_inflate without a context: the file of all valid cases comes back whole and the library's own
    decoder took every block (no zlib fallback: its tables hold the sets that need the most entries); every malformed case, one per file,
    is MSNV_EFORMAT."""
    data, want = dc.valid_file()
    p = str(tmp_path / "valid.gz")
    open(p, "wb").write(data)
    before = _fallbacks()
    got, cnt = core.bgzf_inflate(p)
    assert got.tobytes() == want
    assert _fallbacks() == before
    good = dc.valid_cases()[0]
    for c in dc.malformed_cases():
        q = str(tmp_path / "bad.gz")
        open(q, "wb").write(dc.bgzf([(good.stream, good.intended), (c.stream, c.intended), (good.stream, good.intended)]))
        with pytest.raises(_lib.MsnvError) as e:
            core.bgzf_inflate(q)
        assert e.value.code == _lib.EFORMAT, c.name
