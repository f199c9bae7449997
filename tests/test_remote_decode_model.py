"""The checker of the Beast / AVR input (tests/remote_decode.py) against hand-built known answers from the reference's
rules (net_io.c:1486-1627,2504-2569, mode_s.c:424-555,717-726).  CPU only."""
import pytest

from remote_decode import Checker, frame, hulc
from test_wire_readers import crc24, flipped

DF17 = bytes.fromhex("8D4840D6202CC371C32CE0576098")  # a clean ADS-B squitter of 4840D6
AA = 0x4840D6


def with_parity(body, ap=0):
    """body + the three parity bytes that make the syndrome `ap` (0: a clean PI field)."""
    rem = crc24(body + b"\x00\x00\x00")
    return body + (rem ^ ap).to_bytes(3, "big")


def df11(aa, iid=0):
    return with_parity(bytes([(11 << 3) | 5]) + aa.to_bytes(3, "big"), iid)


def df20(addr):
    return with_parity(bytes([20 << 3, 0x00, 0x1F, 0xB8, 0x20, 0x05, 0x64, 0x1C, 0x30, 0x20, 0x00]), addr)


def df4(addr):
    return with_parity(bytes([4 << 3, 0x00, 0x1F, 0xB8]), addr)


@pytest.fixture
def make(pkg, oracle):
    return lambda nfix=1, mode_ac=0: Checker(pkg, oracle, nfix, mode_ac)


def test_clean_df17_is_accepted_and_adds_its_address(make):
    c = make()
    got = c.beast(frame(ord("3"), DF17, ts=0x0102030405, signal=0xFF), now_ms=1000)
    assert len(got) == 1 and got[0]["addr"] == AA and got[0]["correctedbits"] == 0
    assert got[0]["timestampMsg"] == 0x0102030405 and got[0]["signalLevel"] == 1.0 and got[0]["sysTimestampMsg"] == 1000
    assert bytes(got[0]["msg"]) == DF17 and got[0]["msgbits"] == 112 and got[0]["msgtype"] == 17
    assert c.orc.filter_test(AA) and c.stats["remote_accepted"] == [1, 0, 0]


@pytest.mark.parametrize("nfix,bits,verdict", [
    (0, [40], "bad"), (1, [40], 1), (2, [40], 1),
    (1, [40, 77], "bad"), (2, [40, 77], 2),
    (1, [12], 1),  # the repair changes AA: an unknown address then
])
def test_df17_repairs_under_fix_and_aggressive(make, nfix, bits, verdict):
    c = make(nfix)
    got = c.beast(frame(ord("3"), flipped(DF17, bits)), now_ms=0)
    if verdict == "bad":
        assert len(got) == 0 and c.stats["remote_rejected_bad"] == 1
    elif 8 <= bits[0] <= 31:
        assert len(got) == 0 and c.stats["remote_rejected_unknown_icao"] == 1
        c.beast(frame(ord("3"), DF17), now_ms=0)  # now the address is known
        got = c.beast(frame(ord("3"), flipped(DF17, bits)), now_ms=0)
        assert len(got) == 1 and got[0]["correctedbits"] == 1
    else:
        assert len(got) == 1 and got[0]["correctedbits"] == verdict and bytes(got[0]["msg"]) == DF17
        assert got[0]["crc"] == crc24(flipped(DF17, bits))
        assert not c.orc.filter_test(AA)  # a repaired squitter adds nothing
        assert c.stats["remote_accepted"][verdict] == 1


def test_corrected_df11_of_an_unknown_address(make):
    c = make(1)
    bad = flipped(df11(AA), [20])
    assert len(c.beast(frame(ord("2"), bad), 0)) == 0 and c.stats["remote_rejected_unknown_icao"] == 1
    c.beast(frame(ord("2"), df11(AA)), 0)  # clean, II = 0: accepted and added
    assert c.orc.filter_test(AA)
    got = c.beast(frame(ord("2"), bad), 0)
    assert len(got) == 1 and got[0]["correctedbits"] == 1 and got[0]["addr"] == AA and got[0]["iid"] == 0


def test_df11_with_an_interrogator_code_is_accepted_but_adds_nothing(make):
    c = make(1)
    got = c.beast(frame(ord("2"), df11(AA, iid=5)), 0)
    assert len(got) == 1 and got[0]["iid"] == 5 and not c.orc.filter_test(AA)


def test_df20_exact_match(make):
    c = make(1)
    assert len(c.beast(frame(ord("3"), df20(AA)), 0)) == 0 and c.stats["remote_rejected_unknown_icao"] == 1
    c.beast(frame(ord("3"), DF17), 0)
    got = c.beast(frame(ord("3"), df20(AA)), 0)
    assert len(got) == 1 and got[0]["addr"] == AA and got[0]["msgtype"] == 20


def test_all_zero_frames_are_bad(make):
    c = make(1)
    assert len(c.beast(frame(ord("2"), bytes(7)) + frame(ord("3"), bytes(7) + b"\x01" * 7), 0)) == 0
    assert c.stats["remote_rejected_bad"] == 2 and c.stats["remote_received_modes"] == 2


def test_short_df_in_a_long_frame_and_the_divergence(make):
    c = make(1)
    c.beast(frame(ord("3"), DF17), 0)
    long_df4 = df4(AA) + bytes([0xAB] * 7)  # CRC over the first 56 bits only; the other bytes travel along
    got = c.beast(frame(ord("3"), long_df4), 0)
    assert len(got) == 1 and got[0]["msgbits"] == 56 and bytes(got[0]["msg"]) == long_df4
    got = c.beast(frame(ord("2"), DF17[:7]), 0)  # a 56-bit frame with a 112-bit DF: rejected as bad
    assert len(got) == 0 and c.stats["remote_rejected_bad"] == 1


@pytest.mark.parametrize("pieces,bad", [
    ([b"\x00" * 14], 0), ([b"\x00" * 15], 1), ([b"\x00" * 29], 1), ([b"\x00" * 30], 2),
    ([b"\x00" * 14 + b"\x1ax" + b"\x00" * 14], 1),  # two gaps (0 and 15 bytes), not one of 30
    ([b"\x00" * 14 + hulc(30, fill=0)], 2),  # 'H' with len > 24: the 0x1A is skipped, 33 bytes to the next one
])
def test_garbage_is_charged_per_gap(make, pieces, bad):
    c = make(1)
    c.beast(b"".join(pieces) + frame(ord("3"), DF17), 0)
    assert c.stats["remote_rejected_bad"] == bad and c.stats["remote_accepted"] == [1, 0, 0]


def test_trailing_garbage_is_charged_when_the_next_frame_arrives(make):
    c = make(1)
    c.beast(frame(ord("3"), DF17) + b"\x00" * 10, 0)
    assert c.stats["remote_rejected_bad"] == 0 and c.stats["garbage_bytes"] == 10
    c.beast(b"\x00" * 10 + frame(ord("3"), DF17), 0)
    assert c.stats["remote_rejected_bad"] == 1 and c.stats["garbage_bytes"] == 20


def test_types_1_4_5_h(make):
    c = make(1, mode_ac=1)
    got = c.beast(frame(ord("1"), b"\x12\x34") + frame(ord("4"), bytes(14)) + frame(ord("5"), bytes(14)) + hulc(3), 0)
    assert len(got) == 1 and got[0]["msgtype"] == 32 and got[0]["addr"] == (0x1234 & 0xFF7F) | (1 << 24)
    assert c.stats["other_frames"] == 3 and c.stats["remote_received_modeac"] == 1
    c = make(1, mode_ac=0)
    assert len(c.beast(frame(ord("1"), b"\x12\x34"), 0)) == 0 and c.stats["remote_received_modeac"] == 1


def test_escapes_split_across_calls(make):
    c = make(1)
    stream = frame(ord("3"), DF17, ts=0x1A1A1A1A1A1A, signal=0x1A) * 3
    got = []
    for i in range(len(stream)):
        got.extend(c.beast(stream[i:i + 1], 0))
    assert len(got) == 3 and all(g["timestampMsg"] == 0x1A1A1A1A1A1A for g in got)
