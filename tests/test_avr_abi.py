"""AVR text input (msd_accept_avr, msd_get_avr_stats; msd_avr_reader in libmsd_host.so): exported, declared in
modes_hip.h with the constants and the counter structure as specified, listed in capi.EXPORTS and bound with matching
prototypes (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_accept_avr", "msd_get_avr_stats")


def text(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_exported(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "the library is built by __graft_entry__.build()"
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in NAMES + ("msd_avr_span_bytes", "msd_avr_lookback_bytes", "msd_avr_piece_bytes"):
        assert hasattr(lib, n), n
    host = ctypes.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    for n in ("msd_avr_reader_init", "msd_avr_reader_feed", "msd_avr_parse_line"):
        assert hasattr(host, n), n


def test_declared_and_listed(pkg):
    hdr = text("include", "modes_hip.h")
    assert ("int msd_accept_avr(msd_ctx *ctx, const void *bytes, size_t n, int on_device, uint32_t flags, "
            "uint64_t now_ms, msd_message_fn sink, void *user);") in hdr
    assert "int msd_get_avr_stats(const msd_ctx *ctx, msd_avr_stats *st);" in hdr
    assert "#define MSD_AVR_LINE_MAX 256u" in hdr
    assert "#define MSD_AVR_KEEP_TIMESTAMP 1u" in hdr
    assert pkg.capi.AVR_LINE_MAX == 256 and pkg.capi.AVR_KEEP_TIMESTAMP == 1
    for n in NAMES:
        assert n in pkg.capi.EXPORTS
    wire = text("readsb-protobuf_amd", "csrc", "host", "msd_wire.h")
    assert "void msd_avr_reader_init(msd_avr_reader *r, int mode_ac, int keep_timestamp);" in wire
    assert ("size_t msd_avr_reader_feed(msd_avr_reader *r, const uint8_t *data, size_t n, msd_message_fn fn, "
            "void *user);") in wire


def struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name),
                     open(os.path.join(ROOT, "include", "modes_hip.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(d.split()) for d in body.split(";") if d.strip()]


def test_stats_layouts(pkg):
    """sizeof(msd_avr_stats) == 32 with the header's four counters in order; msd_remote_stats is as it was."""
    S = pkg.capi.AvrStats
    assert ctypes.sizeof(S) == 32
    assert struct_fields("msd_avr_stats") == [("uint64_t", n) for n in ("lines", "frames", "dropped_lines", "long_lines")]
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("lines", 0), ("frames", 8), ("dropped_lines", 16),
                                                                  ("long_lines", 24)]
    assert ctypes.sizeof(pkg.capi.RemoteStats) == 88
    assert struct_fields("msd_remote_stats") == [("uint64_t", n) for n in (
        "remote_received_modes", "remote_received_modeac", "remote_rejected_bad", "remote_rejected_unknown_icao",
        "remote_accepted[3]", "frames", "other_frames", "garbage_bytes", "tile_rewalks")]


def test_prototypes(pkg):
    C = ctypes
    L = pkg.capi.lib()
    f = L.msd_accept_avr
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p,
                                C.c_void_p]
    f = L.msd_get_avr_stats
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.POINTER(pkg.capi.AvrStats)]
    for name in ("accept_avr", "avr_stats"):
        assert callable(getattr(pkg.capi.Demodulator, name, None)), name


def test_kernel_constants(pkg):
    """What the boundary tests derive their offsets from: a workgroup's span and its look-back, which must hold every
    byte that decides where a line starts; the piece of a call."""
    L = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in ("msd_avr_span_bytes", "msd_avr_lookback_bytes", "msd_avr_piece_bytes"):
        getattr(L, n).restype = ctypes.c_uint32
    assert L.msd_avr_lookback_bytes() >= pkg.capi.AVR_LINE_MAX + 1
    assert L.msd_avr_span_bytes() % 64 == 0 and L.msd_avr_lookback_bytes() % 64 == 0
    assert L.msd_avr_piece_bytes() == 1 << 23


def test_null_and_bad_flags_are_refused_without_a_context(pkg):
    import errno
    L = pkg.capi.lib()
    st = pkg.capi.AvrStats()
    assert L.msd_accept_avr(None, b"", 0, 0, 0, 0, None, None) == -errno.EINVAL
    assert L.msd_get_avr_stats(None, C_byref(st)) == -errno.EINVAL


def C_byref(x):
    return ctypes.byref(x)
