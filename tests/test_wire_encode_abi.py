"""Wire output on the GPU (msd_wire_encode, msd_group_submit_device_wire, msd_group_submit_host_wire): declared in
modes_hip.h with their formats, flag and sink type, exported by the library, listed in capi.EXPORTS and bound with matching
prototypes (no GPU needed)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_wire_encode", "msd_group_submit_device_wire", "msd_group_submit_host_wire")


def text(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_declared_and_listed(pkg):
    hdr = text("include", "modes_hip.h")
    assert "enum { MSD_WIRE_BEAST = 0, MSD_WIRE_AVR = 1, MSD_WIRE_AVR_MLAT = 2 };" in hdr
    assert "#define MSD_WIRE_VERBATIM 1u" in hdr
    assert ("int msd_wire_encode(msd_ctx *ctx, const msd_message *msgs, size_t n, int on_device, int format, "
            "uint32_t flags, uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends);") in hdr
    assert ("typedef void (*msd_group_wire_fn)(uint32_t receiver, const uint8_t *bytes, size_t nbytes, "
            "uint32_t nmessages, void *user);") in hdr
    for which, iq in (("device", "d_iq"), ("host", "h_iq")):
        assert (f"int msd_group_submit_{which}_wire(msd_group *g, const void *{iq}, const msd_group_entry *e, uint32_t n, "
                "int format, uint32_t flags, msd_group_wire_fn sink, void *user);") in hdr
    for n in NAMES:
        assert n in pkg.capi.EXPORTS
    capi = pkg.capi
    assert (capi.WIRE_BEAST, capi.WIRE_AVR, capi.WIRE_AVR_MLAT, capi.WIRE_VERBATIM) == (0, 1, 2, 1)


def test_bytes_per_message():
    """MSD_BEAST_MAX bounds what one message takes in every format: the group's output array is sized from it (44 bytes
    per Mode S message, 20 per Mode A/C reply) and the kernels' LDS image holds 256 messages of it."""
    wire_h = text("readsb-protobuf_amd", "csrc", "host", "msd_wire.h")
    beast_max = int(re.search(r"#define MSD_BEAST_MAX (\d+)", wire_h).group(1))
    avr_max = int(re.search(r"#define MSD_AVR_MAX (\d+)", wire_h).group(1))
    assert beast_max == 44 == 2 + 2 * (6 + 1 + 14)      # every byte behind the type byte escaped
    assert 1 + 12 + 2 * 14 + 2 <= beast_max <= avr_max  # the longest AVR line (no NUL) fits as well
    assert 2 + 2 * (6 + 1 + 2) == 20 and 1 + 12 + 2 * 2 + 2 <= 20  # a Mode A/C reply
    impl = text("readsb-protobuf_amd", "csrc", "msd_wire_impl.h")
    assert int(re.search(r"#define MSD_WIRE_MAX (\d+)u", impl).group(1)) == beast_max


def test_exported(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "the library is built by __graft_entry__.build()"
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in NAMES + ("msd_beast_frame_out", "msd_avr_line_out"):  # the host writers are in this library too
        assert hasattr(lib, n), n
    host = ctypes.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    for n in ("msd_beast_frame_out", "msd_avr_line_out", "msd_wire_verbatim"):  # ... and libmsd_host.so keeps its copy
        assert hasattr(host, n), n


def test_prototypes(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "the library is built by __graft_entry__.build()"
    C = ctypes
    L = pkg.capi._group_lib()
    assert L.msd_wire_encode.restype is C.c_int
    assert list(L.msd_wire_encode.argtypes) == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint32,
                                                C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    for n in NAMES[1:]:
        f = getattr(L, n)
        assert f.restype is C.c_int
        assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p,
                                    C.c_void_p]
    sink = pkg.capi._GROUP_WIRE_SINK
    assert sink._restype_ is None
    assert list(sink._argtypes_) == [C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]


def test_python_methods(pkg):
    sig = inspect.signature(pkg.capi.Demodulator.encode_wire)
    assert list(sig.parameters)[1:] == ["messages", "format", "verbatim", "on_device"]
    for name in ("submit_device_wire", "submit_host_wire"):
        assert callable(getattr(pkg.capi.ReceiverGroup, name, None)), name
