"""The read subsampler's rule in plain Python (`qaCompute -a SEED.FRAC`, qaCompute.cpp:319-325, :454-458; the rule of `samtools view -s`):
what csrc/devsub.h states for the host and the device, written a third time with nothing shared.

    name       the record's read name up to its NUL
    x31(name)  h = first byte; if it is non-zero, h = h * 31 + byte for every further byte; uint32; bytes are SIGNED chars
    wang(k)    khash.h's integer mix, uint32
    word       0 for seed 0, else glibc's srand(seed); rand() -- asked of libc itself
    dropped    when (wang(x31(name) ^ word) & 0xffffff) / 0x1000000 >= frac

x31 and wang are restated from memory of htslib's khash.h; nothing here has been compared with a real qaCompute or samtools (DESIGN.md
section 7)."""
import ctypes
import ctypes.util
import struct

M32 = 0xffffffff


def x31(name):
    """name: bytes without the NUL."""
    if not name:
        return 0
    sc = [b - 256 if b >= 128 else b for b in name]
    h = sc[0] & M32
    if h:
        for c in sc[1:]:
            h = (h * 31 + c) & M32
    return h


def wang(k):
    k = (k + (~(k << 15) & M32)) & M32
    k ^= k >> 10
    k = (k + (k << 3)) & M32
    k ^= k >> 6
    k = (k + (~(k << 11) & M32)) & M32
    k ^= k >> 16
    return k


_libc = None


def seed_word(seed):
    """0 for seed 0, else srand(seed); rand() of the C library this process runs on."""
    global _libc
    if seed == 0:
        return 0
    if _libc is None:
        _libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
        _libc.srand.argtypes = [ctypes.c_uint]
        _libc.rand.restype = ctypes.c_int
    _libc.srand(seed & M32)
    return _libc.rand() & M32


def mixed(name, word):
    return wang(x31(name) ^ word)


def keep(name, word, frac):
    """The reference's form: a division and a comparison of doubles."""
    return not ((mixed(name, word) & 0xffffff) / float(0x1000000) >= frac)


def record_name(buf, off):
    l_name = buf[off + 12]
    raw = bytes(buf[off + 36:off + 36 + l_name])
    return raw.split(b"\0", 1)[0]


def split_records(stream):
    """(offset, size) of every record of a raw stream."""
    buf = bytes(stream)
    out, off = [], 0
    while off < len(buf):
        size = struct.unpack_from("<i", buf, off)[0] + 4
        out.append((off, size))
        off += size
    assert off == len(buf)
    return out


def filter_stream(stream, word, frac):
    """(kept bytes, kept count, dropped count); frac <= 0: no subsampling at all."""
    buf = bytes(stream)
    if not frac > 0:
        return buf, len(split_records(buf)), 0
    out, kept, dropped = [], 0, 0
    for off, size in split_records(buf):
        if keep(record_name(buf, off), word, frac):
            out.append(buf[off:off + size]); kept += 1
        else:
            dropped += 1
    return b"".join(out), kept, dropped


def parse_arg(text):
    """-a ARG as qaCompute.cpp:319-325 reads it: strtol(ARG, &q, 10), then strtod(q, &q).  Returns (seed, frac); raises ValueError for a
    seed the product refuses (negative, or above 2^32 - 1: the reference truncates those)."""
    libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.strtol.restype = ctypes.c_long
    libc.strtol.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    libc.strtod.restype = ctypes.c_double
    libc.strtod.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
    buf = ctypes.create_string_buffer(text.encode())
    q = ctypes.c_char_p()
    seed = libc.strtol(buf, ctypes.byref(q), 10)
    frac = libc.strtod(q, None)
    if seed < 0 or seed > M32:
        raise ValueError("subsampling seed %d is outside 0 .. 4294967295" % seed)
    return seed, frac


def with_name(record, name):
    """A record built by bamtools.make_record with a placeholder name of len(name) characters, renamed to the BYTES `name` (any value but 0)."""
    rec = bytearray(record)
    assert rec[12] == len(name) + 1
    rec[36:36 + len(name)] = name
    return bytes(rec)
