"""Verbatim wire output of a group's remote inputs takes the received bytes from the bit positions the CRC repair names
(msd_wire_source(..., have_errbits = true, ...)); the host writers it is held to search for them (msd_wire_verbatim).
This enumerates every correctable error pattern of one and two bits, for 56 and 112 bits, and holds the positions the
repair tables name against the positions the search finds: they are the same in every case, so the search is needed
nowhere (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

from avr_streams import crc24


def syndromes(bits):
    """bit position -> the syndrome of that bit alone, for the positions the repair looks at (crc.c:216)"""
    out = {}
    for i in range(5, bits):
        m = bytearray(bits // 8)
        m[i >> 3] = 0x80 >> (i & 7)
        out[i] = crc24(bytes(m[:-3])) ^ int.from_bytes(m[-3:], "big")
    return out


@pytest.fixture(scope="module")
def libs(pkg):
    L = C.CDLL(pkg.capi.LIB_PATH)
    L.msd_fix2_diagnose.restype = C.c_int
    L.msd_fix2_diagnose.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_int * 2)]
    H = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    H.msd_wire_verbatim.restype = C.c_int
    H.msd_wire_verbatim.argtypes = [C.c_void_p, C.c_void_p]
    return L, H


def searched(pkg, H, bits, syndrome, nbits_wrong, msgtype=17):
    """the positions msd_wire_verbatim flips in an all-zero message that carries this syndrome"""
    m = np.zeros(1, dtype=pkg.capi.MESSAGE_DTYPE)
    m["msgbits"], m["msgtype"], m["correctedbits"], m["crc"] = bits, msgtype, nbits_wrong, syndrome
    out = (C.c_uint8 * 14)()
    n = H.msd_wire_verbatim(m.ctypes.data, out)
    return n, [8 * j + b for j in range(14) for b in range(8) if out[j] & (0x80 >> b)]


@pytest.mark.parametrize("bits", [56, 112])
def test_single_bit_repairs(pkg, libs, bits):
    """--fix: the single-bit syndromes are pairwise different, so the first position the search meets is the repaired
    one; DF11 compares under the mask that leaves the interrogator id out."""
    _, H = libs
    syn = syndromes(bits)
    assert len(set(syn.values())) == len(syn)
    for i, s in syn.items():
        assert searched(pkg, H, bits, s, 1) == (1, [i]), i
    if bits == 56:
        masked = {i: s for i, s in syn.items() if s & 0x7F == 0}  # the positions a DF11 repair can name
        assert len(set(masked.values())) == len(masked) and len(masked) > 0
        for i, s in masked.items():
            assert searched(pkg, H, bits, s | 0x55, 1, msgtype=11) == (1, [i]), i


@pytest.mark.parametrize("bits", [56, 112])
def test_every_pattern_of_the_two_bit_tables(pkg, libs, bits):
    """--aggressive: every syndrome of one or two bits that the table corrects, against the search."""
    L, H = libs
    syn = syndromes(bits)
    pos = sorted(syn)
    one = two = 0
    bit = (C.c_int * 2)()
    for a in pos:
        ne = L.msd_fix2_diagnose(bits, syn[a], C.byref(bit))
        if ne > 0:
            assert ne == 1 and bit[0] == a
            assert searched(pkg, H, bits, syn[a], 1) == (1, [a]), a
            one += 1
        for b in pos:
            if b <= a:
                continue
            s = syn[a] ^ syn[b]
            ne = L.msd_fix2_diagnose(bits, s, C.byref(bit))
            if ne <= 0:
                continue
            assert ne == 2 and sorted((bit[0], bit[1])) == [a, b], (a, b, ne, bit[0], bit[1])
            assert searched(pkg, H, bits, s, 2) == (2, [a, b]), (a, b)
            two += 1
    print(bits, "bits: correctable patterns of one bit", one, "and of two bits", two)
    assert one > 0 and two > 0
