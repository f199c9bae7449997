"""The fields entries of receiver groups: exported by the library, declared in modes_hip.h with their sink type, listed
in capi.EXPORTS and bound by ReceiverGroup with matching prototypes (no GPU needed)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_group_submit_device_fields", "msd_group_submit_host_fields")


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())


def test_declared_and_listed(pkg):
    hdr = header()
    assert ("typedef void (*msd_group_fields_fn)(uint32_t receiver, const msd_message *mm, const msd_fields *fields, "
            "void *user);") in hdr
    assert ("int msd_group_submit_device_fields(msd_group *g, const void *d_iq, const msd_group_entry *e, uint32_t n, "
            "msd_group_fields_fn sink, void *user);") in hdr
    assert ("int msd_group_submit_host_fields(msd_group *g, const void *h_iq, const msd_group_entry *e, uint32_t n, "
            "msd_group_fields_fn sink, void *user);") in hdr
    for n in NAMES:
        assert n in pkg.capi.EXPORTS


def test_exported(pkg):
    if not os.path.exists(pkg.capi.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_prototypes(pkg):
    """The binding's prototypes are those of the header: (group, iq, entries, n, sink, user) -> int, the same as the plain
    entries', and a sink of (uint32 receiver, message, fields, user) -> void."""
    if not os.path.exists(pkg.capi.LIB_PATH):
        pytest.skip("library not built")
    C = ctypes
    L = pkg.capi._group_lib()
    for n in NAMES:
        f = getattr(L, n)
        assert f.restype is C.c_int
        assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        assert list(f.argtypes) == list(getattr(L, n[:-len("_fields")]).argtypes)
    sink = pkg.capi._GROUP_FIELDS_SINK
    assert sink._restype_ is None
    assert list(sink._argtypes_) == [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert C.sizeof(pkg.capi.GroupEntry) == 16


def test_python_methods(pkg):
    G = pkg.capi.ReceiverGroup
    assert "fields" in inspect.signature(G.submit).parameters
    assert callable(getattr(G, "submit_fields", None))
