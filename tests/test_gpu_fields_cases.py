"""The device copies of msd_fields_impl.h on the constructed families of tests/field_cases.py.  msd_decode_fields_device
(the copy of msd_resolve_kernels.hip) on every family: its result equals the second reading (tests/indep_fields.py) member
by member and the host build byte for byte, and the hand-typed answers hold on the device's own result.  Families b and c
also go through msd_group_accept_beast_fields on a one-receiver group, as Beast frames with valid parity, which holds the
copy of msd_group_remote_out_kernels.hip to the same answers.  Every comparison is exact."""
import numpy as np
import pytest

import field_cases as fc
from avr_streams import crc24
from remote_decode import frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dem(pkg, torch_cuda):
    d = pkg.Demodulator(nfix_crc=1, max_batch_samples=131072)
    yield d
    d.close()


def check_device(pkg, dem, letter):
    records, note = fc.build(pkg.capi.MESSAGE_DTYPE, letter)
    assert len(records) <= 1 << 20
    members, source_known, floats, detail = fc.second_reading(records, letter)
    if letter == "g":
        fc.assert_family_g(note, detail)  # on the second reading alone, before anything is compared
    got = dem.decode_fields_device(records)
    fc.assert_members(got, members, source_known, records, "device decode")
    fc.assert_known(got, note, records, "device decode")
    fc.assert_floats(fc.host_floats(pkg, got), floats, records, "msd_fields_to_float of the device's fields")
    host = fc.host_decode(pkg, records)
    if host.tobytes() != got.tobytes():
        bad = np.flatnonzero((host.view(np.uint8).reshape(len(host), -1) != got.view(np.uint8).reshape(len(got), -1)).any(axis=1))
        raise AssertionError("device and host bytes differ in %d records, first %s" % (len(bad), fc.where(records, int(bad[0]))))
    return got


@pytest.mark.parametrize("letter", list("abcdef"))
def test_device_decode_of_a_family(pkg, dem, letter):
    check_device(pkg, dem, letter)


def test_device_decode_of_the_turn_rate_family(pkg, dem):
    """Family g: the device's own tan at the threshold of comm_b.c:552-559 -- the 102 ties, every triple within 1e-2 and
    every 97th of the other 8.4 million, each with BDS 6,0 at 56 so that the penalty decides commb_format 1 against 9.  The
    nearest non-tie is 4.4e-6 from the threshold: a correct tan leaves no triple in doubt."""
    got = check_device(pkg, dem, "g")
    assert int((got["commb_format"] == 1).sum()) >= 10000 and int((got["commb_format"] == 9).sum()) >= 10000


@pytest.mark.parametrize("letter", ["b", "c"])
def test_group_beast_fields_of_a_family(pkg, torch_cuda, letter):
    records, note = fc.build(pkg.capi.MESSAGE_DTYPE, letter)
    assert np.isin(records["msgtype"], (17, 18)).all()
    members, source_known, floats, _ = fc.second_reading(records, letter)
    stream = bytearray()
    for k, m in enumerate(records):
        body = m["msg"][:11].tobytes()
        stream += frame(ord("3"), body + crc24(body).to_bytes(3, "big"), 1000 + k, 0x40)
    g = pkg.capi.ReceiverGroup(1, fmt=pkg.capi.FMT_UC8, nfix_crc=1, flags=pkg.capi.CFG_DECODE_FIELDS)
    try:
        got = g.accept_beast_fields([(0, bytes(stream))], 1)
    finally:
        g.close()
    assert list(got) == [0] and len(got[0]) == len(records)
    msgs = np.array([m for m, _ in got[0]], dtype=pkg.capi.MESSAGE_DTYPE)
    fields = np.array([f for _, f in got[0]], dtype=pkg.capi.FIELDS_DTYPE)
    assert np.array_equal(msgs["msg"][:, :11], records["msg"][:, :11]) and np.array_equal(msgs["addr"], records["addr"])
    assert np.array_equal(msgs["msgtype"], records["msgtype"]) and (msgs["correctedbits"] == 0).all()
    fc.assert_members(fields, members, source_known, records, "group decode")
    fc.assert_known(fields, note, records, "group decode")
    fc.assert_floats(fc.host_floats(pkg, fields), floats, records, "msd_fields_to_float of the group's fields")
    assert fields.tobytes() == fc.host_decode(pkg, msgs).tobytes()
