"""Decoded fields and wire output for the remote inputs of a group (msd_group_accept_beast_fields, _avr_fields,
_beast_wire, _avr_wire): exported by the library, declared in modes_hip.h with their contract, listed in capi.EXPORTS
and bound with matching prototypes (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_group_accept_beast_fields", "msd_group_accept_avr_fields", "msd_group_accept_beast_wire",
         "msd_group_accept_avr_wire")


def text(*path):
    """the file with the comments' line breaks (and their " * ") taken out"""
    return re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", open(os.path.join(ROOT, *path)).read()))


def test_exported(pkg):
    assert os.path.exists(pkg.capi.LIB_PATH), "the library is built by __graft_entry__.build()"
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.capi.EXPORTS


def test_declared(pkg):
    hdr = text("include", "modes_hip.h")
    for kind in ("beast", "avr"):
        assert (f"int msd_group_accept_{kind}_fields(msd_group *g, const void *bytes, int on_device, "
                f"const msd_group_{kind}_entry *e, uint32_t n, msd_group_fields_fn sink, void *user);") in hdr
        assert (f"int msd_group_accept_{kind}_wire(msd_group *g, const void *bytes, int on_device, "
                f"const msd_group_{kind}_entry *e, uint32_t n, int format, uint32_t flags, msd_group_wire_fn sink, "
                "void *user);") in hdr
    for clause in ("*fields == msd_decode_fields(mm, NULL, ...)", "carry is always NULL, also for Mode A/C records",
                   "must have been created with MSD_CFG_DECODE_FIELDS",
                   "The sink is called exactly once per entry, in entry order",
                   "nmessages is the number of those records, forwarded or not",
                   "A record with correctedbits == 2 produces bytes only with MSD_WIRE_VERBATIM",
                   "A group may mix all six accept calls and all six submit calls",
                   "-EINVAL for an unknown format or flag bit, with the group's state untouched",
                   "Every error leaves the group's state untouched",
                   "no synchronisation beyond the two a piece has", "140 bytes", "44 bytes (MSD_WIRE_MAX)"):
        assert clause in hdr, clause


def test_prototypes(pkg):
    C = ctypes
    L = pkg.capi._group_lib()
    for kind, E in (("beast", pkg.capi.GroupBeastEntry), ("avr", pkg.capi.GroupAvrEntry)):
        f = getattr(L, f"msd_group_accept_{kind}_fields")
        assert f.restype is C.c_int
        assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(E), C.c_uint32, C.c_void_p, C.c_void_p]
        f = getattr(L, f"msd_group_accept_{kind}_wire")
        assert f.restype is C.c_int
        assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(E), C.c_uint32, C.c_int, C.c_uint32,
                                    C.c_void_p, C.c_void_p]
        for name in (f"accept_{kind}_fields", f"accept_{kind}_wire"):
            assert callable(getattr(pkg.capi.ReceiverGroup, name, None)), name
