"""The MSNV_* environment knobs are declared once -- csrc/knobs.h for the library, metasnv_amd/knobs.py for the Python host -- and
KERNELS.md "Environment knobs" has a row for every one: source scans in the style of test_abi.py, and the parsing of a knob of every
kind through tests/native/knobs_harness.cpp (g++ and knobs.h alone; no GPU).

The expected values of the parsing tests are written out by hand from the expressions the call sites held before knobs.h (quoted
beside each table); they are pure functions of the raw string.  atoi("99999999999") is glibc's (int)strtol = 1215752191."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metasnv_amd", "csrc")
NAME = r"MSNV_[A-Z0-9_]+"


def _read(*parts):
    return open(os.path.join(ROOT, *parts), errors="replace").read()


def _header_names():
    return re.findall(r'"(%s)"' % NAME, _read("metasnv_amd", "csrc", "knobs.h"))


def _python_names():
    return re.findall(r'"(%s)"' % NAME, re.sub(r'""".*?"""', "", _read("metasnv_amd", "knobs.py"), flags=re.S))


def _table_names():
    text = _read("KERNELS.md")
    section = text[text.index("## Environment knobs"):]
    section = section[:section.index("\n## ", 1)]
    return re.findall(r"^\| `(%s)` \|" % NAME, section, re.M)


def test_getenv_is_called_in_knobs_h_only():
    hits = [os.path.basename(p) for ext in ("cpp", "hip", "h") for p in glob.glob(os.path.join(CSRC, "*." + ext)) if "getenv" in open(p, errors="replace").read()]
    assert hits == ["knobs.h"]


def test_python_looks_msnv_names_up_in_knobs_py_only():
    for dp, _, files in os.walk(os.path.join(ROOT, "metasnv_amd")):
        for f in files:
            if f.endswith(".py") and f != "knobs.py":
                for i, line in enumerate(open(os.path.join(dp, f), errors="replace"), 1):
                    assert not re.search(r"(environ|getenv).*MSNV_", line), "%s:%d" % (os.path.join(dp, f), i)


def test_every_name_is_one_literal():
    for names in (_header_names(), _python_names()):
        assert len(names) > 10
        assert sorted(names) == sorted(set(names)), [n for n in set(names) if names.count(n) > 1]


def test_the_table_of_kernels_md_lists_exactly_the_declared_names():
    declared = set(_header_names()) | set(_python_names()) | {"MSNV_EXIT"}           # (metaSNV.py's own: read before the package is imported)
    table = _table_names()
    assert sorted(table) == sorted(set(table)), "a name has two rows"
    assert declared == set(table), (sorted(declared - set(table)), sorted(set(table) - declared))
    assert '"MSNV_EXIT"' in _read("metaSNV.py")


# MSNV_* names under tests/ that are not knobs of the product: what only bench.py or the tests themselves read
NOT_KNOBS = {
    "MSNV_STRONG_EXTRA_LIMIT_S",                                     # bench.py's own
    "MSNV_SAMTOOLS",                                                 # tests/reftools.py: where samtools is
    "MSNV_GUARD_DEBUG",                                              # tests/_guard_worker.py: prints its cohorts
    "MSNV_FULL_CONFIG3_SCALE", "MSNV_FULL_CONFIG4_SCALE", "MSNV_SKIP_FULL_CONFIG3", "MSNV_SKIP_FULL_CONFIG4",      # tests/test_gpu_full_config3.py: its own size and skip switches
}


def test_every_name_a_test_sets_is_declared():
    """A test that sets a name the product does not read forces nothing.  "Sets": NAME=... as a keyword, or the quoted name as a key, an
    index, an argument or a list item (dict(os.environ, NAME=...), {"NAME": ...}, os.environ["NAME"], setenv("NAME", ...), knob lists)."""
    declared = set(_header_names()) | set(_python_names()) | {"MSNV_EXIT"} | NOT_KNOBS
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.basename(p) == "test_knobs.py":
            continue
        text = open(p, errors="replace").read()
        used = set(re.findall(r"\b(%s)\s*=[^=]" % NAME, text)) | set(re.findall(r"[\"'](%s)[\"']\s*[:\],]" % NAME, text))
        assert used <= declared, (os.path.basename(p), sorted(used - declared))


# ---------------------------------------------------------------------------------- parsing
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knobs") / "knobs_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "knobs_harness.cpp"), "-o", exe])

    def run(accessor, env, then=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith("MSNV_")}
        e.update(env)
        r = subprocess.run([exe, accessor] + list(then or ()), capture_output=True, text=True, env=e, timeout=60)
        assert r.returncode == 0, r.stderr
        return r.stdout.split("\n")[:-1]
    return run


BIG = "99999999999"
ATOI_BIG = "1215752191"
RAW = (None, "", "0", "1", "-5", "abc", BIG)                       # None: unset

# accessor: (variable, what RAW gives, {further raw strings: what they give})
PARSING = {
    # e && e[0] == 'h'
    "pack_on_host": ("MSNV_PACK", "0000000", {"host": "1", "h": "1", "device": "0", "Host": "0"}),
    # e && e[0] == '0'
    "lean_off": ("MSNV_LEAN", "0010000", {"00": "1", "off": "0"}),
    # !(e && e[0] == '0')
    "item_taper": ("MSNV_ITEM_TAPER", "1101111", {}),
    # e && e[0] == '1'
    "merge_always": ("MSNV_MERGE_ALWAYS", "0001000", {"10": "1", "yes": "0"}),
    "guard_alloc": ("MSNV_GUARD_ALLOC", "0001000", {"10": "1"}),
    "finalize_trace": ("MSNV_FINALIZE_TRACE", "0001000", {}),
    # e && e[0] == 'm' / 't'
    "depth_on_main": ("MSNV_DEPTH_STREAM", "0000000", {"main": "1", "own": "0"}),
    "crc_table": ("MSNV_CRC", "0000000", {"table": "1", "clmul": "0"}),
    # !e ? 0 : e[0] == 'b' ? 1 : e[0] == 'w' ? 2 : 0
    "merged_gather": ("MSNV_MERGED_GATHER", "0000000", {"block": "1", "wave": "2", "both": "1"}),
    # if (e && e[0] == 'p') ...; if (e && e[0] == 'd') ...; else by the dataset
    "layout": ("MSNV_LAYOUT", "-------", {"pieces": "p", "dense": "d", "p": "p"}),
    # !(fe && fe[0] == '0') && (sparse || (fe && fe[0] == '1'))
    "fuse": ("MSNV_FUSE", "--01---", {"10": "1"}),
    # e[0] == 'd' ? ... : e[0] == 's' ? false : <by the dataset>
    "cov_index": ("MSNV_COV_INDEX", "-------", {"dense": "d", "sort": "s"}),
    # e[0] == 's' / e[0] == 'n'
    "stage_free": ("MSNV_STAGE_FREE", "-------", {"sync": "s", "never": "n", "threads": "-"}),
    # if (e) planes = e[0] == 'p'
    "alleles": ("MSNV_ALLELES", "-eeeeee", {"planes": "p", "events": "e"}),
    # if (e) return e[0] == 'd'
    "inflate_where": ("MSNV_INFLATE", "-hhhhhh", {"device": "d", "host": "h", "zlib": "h"}),
    # e && e[0] == 'z'
    "inflate_zlib": ("MSNV_INFLATE", "0000000", {"zlib": "1", "host": "0", "device": "0"}),
    # getenv(...) != nullptr
    "cov_late": ("MSNV_COV_LATE", "0111111", {}),
    "no_adopt": ("MSNV_NO_ADOPT", "0111111", {}),
    "debug_sync": ("MSNV_DEBUG_SYNC", "0111111", {}),
    # v = e ? atoi(e) : 1; v < 0 ? 0 : v
    "inflate_check_every": ("MSNV_INFLATE_CHECK", ["1", "0", "0", "1", "0", "0", ATOI_BIG], {"7": "7"}),
    # v = e ? atoll(e) : (res ? 2048 : 1024); max(1, v) << 20
    "inflate_batch_bytes": ("MSNV_INFLATE_BATCH_MB", ["1073741824"] + ["1048576"] * 5 + ["104857599998951424"], {"64": "67108864"}),
    "inflate_batch_bytes_resident": ("MSNV_INFLATE_BATCH_MB", ["2147483648"] + ["1048576"] * 5 + ["104857599998951424"], {"64": "67108864"}),
    # x = e ? atoi(e) : 192; min(NARROW_MAX_DEPTH, max(32, x)) -- the harness passes 255 for the bound
    "split_at_255": ("MSNV_SPLIT_AT", ["192"] + ["32"] * 5 + ["255"], {"40": "40", "300": "255"}),
    # x = e ? atoi(e) : 128; min(250, max(16, x))
    "group_depth": ("MSNV_GROUP_DEPTH", ["128"] + ["16"] * 5 + ["250"], {"24": "24"}),
    # v = e ? atoi(e) : 48; max(0, v)
    "shallow_pieces": ("MSNV_SHALLOW_PIECES", ["48", "0", "0", "1", "0", "0", ATOI_BIG], {}),
    # max(1, e ? atoi(e) : 256)
    "fuse_pieces": ("MSNV_FUSE_PIECES", ["256", "1", "1", "1", "1", "1", ATOI_BIG], {"4096": "4096"}),
    # target = 2000; if (e) target = max<uint64_t>(64, (uint64_t)atoll(e))
    "item_pieces": ("MSNV_ITEM_PIECES", ["2000", "64", "64", "64", "18446744073709551611", "64", BIG], {"100": "100"}),
    # e ? min(2, max(0, atoi(e))) : 0
    "tot_mode_min": ("MSNV_TOT_MODE", ["0", "0", "0", "1", "0", "0", "2"], {"2": "2"}),
    # v = e ? atoll(e) : 16384; (uint32_t)min(v > 0 ? v : 16384, 0x7fffffff) -- devfin.hip's form, the stricter of the two
    "cov_item_intervals": ("MSNV_COV_ITEM", ["16384", "16384", "16384", "1", "16384", "16384", "2147483647"], {"64": "64"}),
    # v = e ? atoll(e) : 32767; min(32767, max(1, v))
    "cov_narrow_max": ("MSNV_COV_NARROW_MAX", ["32767", "1", "1", "1", "1", "1", "32767"], {"100": "100"}),
    # v = e ? atoll(e) : 4096 (scan_sub_walk) / 6144 (a round's one walk); min(32768, max(64, v))
    "scan_sub_bytes_streams": ("MSNV_SCAN_SUB", ["4096"] + ["64"] * 5 + ["32768"], {"256": "256"}),
    "scan_sub_bytes_round": ("MSNV_SCAN_SUB", ["6144"] + ["64"] * 5 + ["32768"], {"256": "256"}),
    # v = e ? atoll(e) : 256; max(1, v) << 10
    "scan_seg_bytes": ("MSNV_SCAN_SEG_KB", ["262144"] + ["1024"] * 5 + ["102399999998976"], {}),
    # v = e ? atoll(e) : 6144; max(1, v) << 20
    "pack_round_bytes": ("MSNV_PACK_ROUND_MB", ["6442450944"] + ["1048576"] * 5 + ["104857599998951424"], {}),
    # e ? atoi(e) : 1
    "huge_pages": ("MSNV_HUGE", ["1", "0", "0", "1", "-5", "0", ATOI_BIG], {"2": "2"}),
    # e ? (uint32_t)atoi(e) : 0
    "tail_skip": ("MSNV_TAIL_SKIP", ["0", "0", "0", "1", "4294967291", "0", ATOI_BIG], {}),
    # e ? max(0, atoll(e)) : -1
    "dev_cache_mb": ("MSNV_DEV_CACHE_MB", ["-1", "0", "0", "1", "0", "0", BIG], {}),
    # e ? max(1, atoi(e)) : 1
    "text_repeat": ("MSNV_TEXT_REPEAT", ["1", "1", "1", "1", "1", "1", ATOI_BIG], {"3": "3"}),
    # max(0, e ? atoll(e) : 0): 0 = no cap (new with stagedev.h: written from the accessor's comment, not from an earlier site)
    "stage_slab_rows": ("MSNV_STAGE_SLAB_ROWS", ["0", "0", "0", "1", "0", "0", BIG], {"7": "7"}),
    # if (e) gather_split = max(1, atoi(e)) -- over the dataset's 2
    "gather_split_2": ("MSNV_GATHER_SPLIT", ["2", "1", "1", "1", "1", "1", ATOI_BIG], {"4": "4"}),
    # if (e) chunk_cap = max(0, atoll(e)) -- over the dataset's 777
    "chunk_cap_777": ("MSNV_CHUNK_CAP", ["777", "0", "0", "1", "0", "0", BIG], {}),
    # if (e) cap_events = (uint32_t)max<long long>(EV_LISTS, atoll(e)) -- over the dataset's 1000, EV_LISTS = 64 here
    "cap_events_1000_min_64": ("MSNV_CAP_EVENTS", ["1000", "64", "64", "64", "64", "64", ATOI_BIG], {"4096": "4096"}),
    # if (e) tiles_per_wg = min(GATE_MAX_TILES, max(1, atoi(e))) -- over the pass's 4, GATE_MAX_TILES = 8 here
    "gate_tiles_4_max_8": ("MSNV_GATE_TILES", ["4", "1", "1", "1", "1", "1", "8"], {"3": "3"}),
    # e ? max(1, atoi(e)) : SCATTER_BLOCKS_PER_LIST -- 16 here
    "scatter_blocks_16": ("MSNV_SCATTER_BLOCKS", ["16", "1", "1", "1", "1", "1", ATOI_BIG], {"64": "64"}),
    # if (e) chunk_bytes = max<uint64_t>(1, (uint64_t)atoll(e)) -- over the call's 4096
    "text_chunk_bytes_4096": ("MSNV_TEXT_CHUNK", ["4096", "1", "1", "1", "18446744073709551611", "1", BIG], {"300": "300"}),
    # if (e) hipMemset(..., atoi(e), ...)
    "guard_fill": ("MSNV_GUARD_FILL", ["-", "0", "0", "1", "-5", "0", ATOI_BIG], {"255": "255"}),
    # u1 = 1.8, u2 = 0.73, u3 = 0.27; if (e) sscanf(e, "%lf,%lf,%lf", &u1, &u2, &u3)
    "taper_at": ("MSNV_TAPER_AT", ["1.8,0.73,0.27", "1.8,0.73,0.27", "0,0.73,0.27", "1,0.73,0.27", "-5,0.73,0.27", "1.8,0.73,0.27", "1e+11,0.73,0.27"],
                 {"1,2,3": "1,2,3", "0.5,0.25": "0.5,0.25,0.27"}),
}


@pytest.mark.parametrize("accessor", sorted(PARSING))
def test_an_accessor_returns_what_its_sites_returned(harness, accessor):
    var, by_raw, more = PARSING[accessor]
    cases = list(zip(RAW, by_raw)) + list(more.items())
    assert len(by_raw) == len(RAW)
    for raw, want in cases:
        got = harness(accessor, {} if raw is None else {var: raw})
        assert got == [want], (var, raw, got, want)


# a second call after setenv: a per-call knob sees it, a once-per-process knob does not
PER_CALL = [("pack_on_host", "MSNV_PACK", "host", "0", "1"), ("inflate_where", "MSNV_INFLATE", "device", "-", "d"), ("cov_late", "MSNV_COV_LATE", "1", "0", "1"),
            ("split_at_255", "MSNV_SPLIT_AT", "40", "192", "40"), ("group_depth", "MSNV_GROUP_DEPTH", "24", "128", "24"), ("cov_narrow_max", "MSNV_COV_NARROW_MAX", "1", "32767", "1"),
            ("scan_sub_bytes_round", "MSNV_SCAN_SUB", "256", "6144", "256"), ("chunk_cap_777", "MSNV_CHUNK_CAP", "5", "777", "5"), ("taper_at", "MSNV_TAPER_AT", "1,2,3", "1.8,0.73,0.27", "1,2,3"),
            ("inflate_check_every", "MSNV_INFLATE_CHECK", "0", "1", "0"), ("guard_fill", "MSNV_GUARD_FILL", "255", "-", "255"), ("merged_gather", "MSNV_MERGED_GATHER", "block", "0", "1"),
            ("stage_slab_rows", "MSNV_STAGE_SLAB_ROWS", "5", "0", "5")]
ONCE = [("guard_alloc", "MSNV_GUARD_ALLOC", "1", "0"), ("inflate_zlib", "MSNV_INFLATE", "zlib", "0"), ("debug_sync", "MSNV_DEBUG_SYNC", "1", "0"),
        ("depth_on_main", "MSNV_DEPTH_STREAM", "main", "0"), ("scatter_blocks_16", "MSNV_SCATTER_BLOCKS", "64", "16"), ("finalize_trace", "MSNV_FINALIZE_TRACE", "1", "0"),
        ("crc_table", "MSNV_CRC", "table", "0"), ("huge_pages", "MSNV_HUGE", "2", "1"), ("tail_skip", "MSNV_TAIL_SKIP", "3", "0"), ("dev_cache_mb", "MSNV_DEV_CACHE_MB", "5", "-1")]


def test_a_per_call_knob_sees_a_change_inside_the_process(harness):
    for accessor, var, value, first, second in PER_CALL:
        assert harness(accessor, {}, (var, value)) == [first, second], accessor


def test_a_once_per_process_knob_keeps_its_first_reading(harness):
    for accessor, var, value, first in ONCE:
        assert harness(accessor, {}, (var, value)) == [first, first], accessor
    assert harness("guard_alloc", {"MSNV_GUARD_ALLOC": "1"}, ("MSNV_GUARD_ALLOC", "0")) == ["1", "1"]
