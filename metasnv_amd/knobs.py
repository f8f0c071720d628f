"""Every MSNV_* environment knob the Python host reads, declared once: the only module under metasnv_amd/ that looks one up in
os.environ (tests/test_knobs.py holds it to that, and to the table of KERNELS.md "Environment knobs").  The library's own knobs are in
csrc/knobs.h; a name read on both sides has the same meaning here, and a default stated on both sides names its accessor there.

All of them are read per call, except `library()`, which _lib.py asks once at import.  What counts as "on" is what each site always
took: a first letter (MSNV_PACK=host and =h are the same), the exact strings "1" / "0", or int() of the value."""
import os


def _get(name, default=None):
    return os.environ.get(name, default)


# ---- the library and the process group (_lib.py, parallel.py)
def library():
    """MSNV_LIBRARY: path of the libmsnv.so to load instead of the one beside the package ('' = unset; developer A/B of two builds,
    profiles/ab.sh).  Profiling only."""
    return _get("MSNV_LIBRARY") or ""


def dist_force():
    """MSNV_DIST_FORCE=1: a process group of ONE rank, so that the RCCL code paths run on a box with a single GPU (tests/_nccl_worker.py)."""
    return _get("MSNV_DIST_FORCE") == "1"


def dist_backend_nccl():
    """MSNV_DIST_BACKEND (nccl): anything else, such as gloo, rehearses the multi-rank path on a box with fewer GPUs than ranks
    (tests/test_gpu_nccl.py, tests/test_gpu_parity.py, bench.py)."""
    return _get("MSNV_DIST_BACKEND", "nccl") == "nccl"


# ---- the all-to-all of record bytes (parallel.py)
def a2a_selfcheck():
    """MSNV_A2A_SELFCHECK=0: skip the first exchange's check of the collective against a known pattern.  Profiling only."""
    return _get("MSNV_A2A_SELFCHECK", "1") != "0"


def a2a_slice_bytes():
    """MSNV_A2A_SLICE_KB (0 = by the world size): kilobytes per slice of the exchange (tests/test_parallel.py)."""
    return int(_get("MSNV_A2A_SLICE_KB", "0")) << 10


def a2a_lists():
    """MSNV_A2A_FORM (lists): anything else exchanges one flat buffer instead of per-rank lists.  Profiling only."""
    return _get("MSNV_A2A_FORM", "lists") == "lists"


# ---- where the stages run (parallel.py, cli.py): the same names, first letters and defaults as csrc/knobs.h
def pack_on_host():
    """MSNV_PACK=host: records are packed by the host stage (csrc/knobs.h: pack_on_host; tests/test_gpu_devpack.py, bench.py)."""
    return _get("MSNV_PACK", "device")[:1] == "h"


def deal_on_host():
    """MSNV_DEAL=host: a round's records are dealt to their owners by the host, not by the device (tests/test_gpu_nccl.py)."""
    return _get("MSNV_DEAL", "device")[:1] == "h"


def inflate_where(unset=""):
    """MSNV_INFLATE=device|host|zlib: the first letter; `unset` is what an unset variable counts as -- '' where the caller then
    estimates as the library does (csrc/knobs.h: inflate_where), "d" in the N-rank feed (tests/test_gpu_inflate.py, bench.py)."""
    return _get("MSNV_INFLATE", unset)[:1]


def inflate_batch_mb():
    """MSNV_INFLATE_BATCH_MB (1024): compressed megabytes per batch of the device inflate -- the 1024 of csrc/knobs.h:
    inflate_batch_bytes (tests/test_gpu_inflate.py)."""
    return int(_get("MSNV_INFLATE_BATCH_MB", "1024"))


def oneshot():
    """MSNV_ONESHOT=device|host: the one-process CLI waits for the context and inflates on the device / never does; '' = by the host's
    cores and the BAMs' size.  Profiling only."""
    return _get("MSNV_ONESHOT", "")[:1]


# ---- the N-rank feed (parallel.py)
def stage_max_bytes():
    """MSNV_STAGE_MAX_MB (0 = no limit of its own): megabytes of BAM files a rank stages in one go.  Profiling only."""
    return int(_get("MSNV_STAGE_MAX_MB", "0")) << 20


def feed_batch():
    """MSNV_FEED_BATCH (0 or '' = by the files' sizes; else at least 1): files a rank decodes per round (profiles/r06_feed_batch.sh).
    Profiling only."""
    v = _get("MSNV_FEED_BATCH")
    return max(1, int(v)) if v else 0


def plan_bytes():
    """MSNV_PLAN_MB (0 = a quarter of the host memory divided by the ranks): megabytes of record bytes a rank holds while the contig
    owners are planned (tests/test_gpu_nccl.py)."""
    return int(_get("MSNV_PLAN_MB", "0")) << 20


def feed_overlap():
    """MSNV_FEED_OVERLAP=0: decode round k + 1 only after round k has been exchanged and packed (tests/test_parallel.py; bench.py's
    strong mode)."""
    return _get("MSNV_FEED_OVERLAP", "1") != "0"


# ---- the CLI (cli.py)
def metrics_path():
    """MSNV_METRICS: file the CLI appends its run metrics to ('' or unset = none; bench.py)."""
    return _get("MSNV_METRICS")
