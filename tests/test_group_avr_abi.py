"""AVR text input per receiver of a group (msd_group_accept_avr, msd_group_get_avr_stats): exported by the library,
declared in modes_hip.h with the entry structure, listed in capi.EXPORTS and bound with matching prototypes; the entry
array the Python wrapper builds from a dict and from a list (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_group_accept_avr", "msd_group_get_avr_stats")


def text(*path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read())


def test_exported(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "the library is built by __graft_entry__.build()"
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_declared_and_listed(pkg):
    hdr = text("include", "modes_hip.h")
    assert ("int msd_group_accept_avr(msd_group *g, const void *bytes, int on_device, const msd_group_avr_entry *e, "
            "uint32_t n, msd_group_message_fn sink, void *user);") in hdr
    assert "int msd_group_get_avr_stats(const msd_group *g, uint32_t receiver, msd_avr_stats *st);" in hdr
    assert "#define MSD_GROUP_AVR_ENTRY_MAX (1u << 20)" in hdr
    assert "#define MSD_GROUP_AVR_OFFSET_MAX ((uint64_t)1 << 47)" in hdr
    assert pkg.capi.GROUP_AVR_ENTRY_MAX == 1 << 20
    for n in NAMES:
        assert n in pkg.capi.EXPORTS


def test_entry_layout(pkg):
    """sizeof(msd_group_avr_entry) == 32, and the header's fields in the header's order at the offsets of
    capi.GroupAvrEntry."""
    E = pkg.capi.GroupAvrEntry
    assert ctypes.sizeof(E) == 32
    want = [("receiver", "uint32_t", 0), ("flags", "uint32_t", 4), ("offset", "uint64_t", 8), ("nbytes", "uint32_t", 16),
            ("reserved", "uint32_t", 20), ("now_ms", "uint64_t", 24)]
    body = re.search(r"typedef struct msd_group_avr_entry \{(.*?)\} msd_group_avr_entry;",
                     open(os.path.join(ROOT, "include", "modes_hip.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [tuple(d.split()) for d in body.split(";") if d.strip()]
    assert decl == [(t, n) for n, t, _ in want]
    sizes = {"uint32_t": 4, "uint64_t": 8}
    assert [(n, getattr(E, n).offset, getattr(E, n).size) for n, _ in E._fields_] == [(n, o, sizes[t]) for n, t, o in want]


def test_prototypes(pkg):
    C = ctypes
    L = pkg.capi._group_lib()
    f = L.msd_group_accept_avr
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(pkg.capi.GroupAvrEntry), C.c_uint32,
                                C.c_void_p, C.c_void_p]
    f = L.msd_group_get_avr_stats
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.c_uint32, C.POINTER(pkg.capi.AvrStats)]
    for name in ("accept_avr", "avr_stats", "avr_entries"):
        assert callable(getattr(pkg.capi.ReceiverGroup, name, None)), name


def fields(e):
    return (e.receiver, e.flags, e.offset, e.nbytes, e.reserved, e.now_ms)


def test_wrapper_builds_the_entry_array(pkg):
    G = pkg.capi.ReceiverGroup
    keep = pkg.capi.AVR_KEEP_TIMESTAMP
    ent, n, data = G.avr_entries({3: b"*ab;", 0: b"", 7: bytearray(b"\n\n")}, 99)
    assert n == 3 and data == b"*ab;\n\n"
    assert [fields(ent[i]) for i in range(n)] == [(3, 0, 0, 4, 0, 99), (0, 0, 4, 0, 0, 99), (7, 0, 4, 2, 0, 99)]
    ent, n, data = G.avr_entries([(1, b"xy"), (0, b"z")], [5, 1 << 40], keep_timestamp=True)
    assert n == 2 and data == b"xyz"
    assert [fields(ent[i]) for i in range(n)] == [(1, keep, 0, 2, 0, 5), (0, keep, 2, 1, 0, 1 << 40)]
    ent, n, data = G.avr_entries([], 0)
    assert n == 0 and data == b""
    try:
        G.avr_entries([(0, b"a")], [1, 2])
    except ValueError:
        pass
    else:
        raise AssertionError("one now_ms per entry")
