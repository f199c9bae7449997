"""The per-receiver Mode A/C entries of receiver groups: exported by the library, declared in modes_hip.h, listed in
capi.EXPORTS and bound by ReceiverGroup (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_group_set_receiver_mode_ac", "msd_group_get_receiver_mode_ac")


def test_declared_and_listed(pkg):
    hdr = open(os.path.join(ROOT, "include", "modes_hip.h")).read()
    assert re.search(r"int msd_group_set_receiver_mode_ac\(msd_group \*g, uint32_t receiver, int on\);", hdr)
    assert re.search(r"int msd_group_get_receiver_mode_ac\(const msd_group \*g, uint32_t receiver, int \*on\);", hdr)
    for n in NAMES:
        assert n in pkg.capi.EXPORTS


def test_exported(pkg):
    if not os.path.exists(pkg.capi.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_python_methods(pkg):
    G = pkg.capi.ReceiverGroup
    assert callable(getattr(G, "set_receiver_mode_ac", None))
    assert callable(getattr(G, "receiver_mode_ac", None))
