"""The field decoder against a second reading (tests/indep_fields.py, written from the reference's lines alone) on the
constructed families of tests/field_cases.py and on random payloads: the host build of msd_fields_impl.h, the second
reading and the oracle agree member by member, msd_fields_to_float of the decoded fields gives the reading's floats bit
for bit, and the hand-typed answers hold for both."""
import numpy as np
import pytest

import field_cases as fc
from test_fields import FIELD_NAMES


def check(pkg, oracle, records, key, note=None):
    members, source_known, floats, detail = fc.second_reading(records, key)
    host = fc.host_decode(pkg, records)
    fc.assert_members(host, members, source_known, records, "host decode")
    orc = fc.oracle_decode(oracle, records)
    fc.assert_members(orc, members, source_known, records, "oracle")
    fc.assert_same_members(host, orc, FIELD_NAMES, records, "host decode against the oracle")
    fc.assert_floats(fc.host_floats(pkg, host), floats, records, "msd_fields_to_float")
    if note:
        fc.assert_known(host, note, records, "host decode")
        want = np.zeros(len(records), dtype=[(n, "S8" if n == "callsign" else "<i8") for n in FIELD_NAMES])
        for n in FIELD_NAMES:
            want[n] = members[n]
        fc.assert_known(want, note, records, "second reading")
    return members, detail


@pytest.mark.parametrize("letter", list("abcdef"))
def test_family(pkg, oracle, letter):
    records, note = fc.build(pkg.capi.MESSAGE_DTYPE, letter)
    assert len(note["known"]) > 0
    check(pkg, oracle, records, letter, note)


def test_family_f_as_one_buffer_with_the_carry(pkg):
    """The same replies as one sample buffer's: each decoded with the one before as its carry, as msd_fields_batch does."""
    import indep_fields
    records, _ = fc.build(pkg.capi.MESSAGE_DTYPE, "f")
    members, source_known = indep_fields.members_of(indep_fields.read(records, one_buffer=True))
    host = np.zeros(len(records), dtype=pkg.capi.FIELDS_DTYPE)
    for i, m in enumerate(records):
        host[i] = pkg.capi.decode_fields(m, host[i - 1] if i else None)
    fc.assert_members(host, members, source_known, records, "host decode with carry")
    kept = (host["altitude_baro_valid"] == 1) & (fc.host_decode(pkg, records)["altitude_baro_valid"] == 0)
    assert kept.sum() > 1000


def test_family_g_turn_rate_check(pkg, oracle):
    """The one libm call of the decoder: every triple of the observable subspace that is a tie or within 1e-2 of the
    threshold, and every 97th of the rest.  8 382 010 triples, 102 ties, 21 149 more within 1e-2 (2 034 within 1e-3), the
    nearest non-tie 4.4e-6 away: no triple is left out."""
    records, note = fc.build(pkg.capi.MESSAGE_DTYPE, "g")
    assert len(records) <= 1 << 20
    members, source_known, floats, detail = fc.second_reading(records, "g")
    ambiguous, unique = fc.assert_family_g(note, detail)  # on the second reading alone, before anything is compared
    assert int((members["commb_format"] == 1).sum()) == ambiguous and int((members["commb_format"] == 9).sum()) == unique
    check(pkg, oracle, records, "g")


def test_random_payloads(pkg, oracle):
    records = fc.random_payloads(pkg.capi.MESSAGE_DTYPE)
    members, _ = check(pkg, oracle, records, "random")
    assert len(records) == 20000 and len(np.unique(members["commb_format"])) >= 3


def test_second_reading_on_the_published_examples(pkg):
    """The reading itself against values from the public ADS-B decoding literature (J. Sun, 'The 1090 MHz riddle'), so that
    it is held to something besides the decoders it judges."""
    raws = [bytes.fromhex(h) for h in ("8D4840D6202CC371C32CE0576098", "8D40621D58C382D690C8AC2863A7", "8D485020994409940838175B284F",
                                      "8DA05F219B06B6AF189400CBC33F", "A000139381951536E024D4CCF6B5", "A00004128F39F91A7E27C46ADC21",
                                      "A000029C85E42F313000007047D3", "8DA05629EA21485CBF3F8CADAEEB")]
    records = fc.to_records(pkg.capi.MESSAGE_DTYPE, raws)
    m, _, f, _ = fc.second_reading(records)
    assert m["callsign"][0] == b"KLM1023 " and m["category"][0] == 0xA0
    assert (m["altitude_baro"][1], m["cpr_lat"][1], m["cpr_lon"][1], m["cpr_odd"][1]) == (38000, 93000, 51372, 0)
    assert (m["ew_vel"][2], m["ns_vel"][2], m["geom_rate"][2], m["geom_delta"][2]) == (-8, -159, -832, 550)
    assert abs(f["gs_selected"][2] - 159.20) < 0.01 and abs(f["heading"][2] - 182.88) < 0.01
    assert abs(f["heading"][3] - 243.98) < 0.01 and (m["tas"][3], m["baro_rate"][3]) == (375, -2304)
    assert (m["commb_format"][4], round(float(f["roll"][4]), 1), float(f["heading"][4]), float(f["gs_selected"][4]),
            float(f["track_rate"][4]), m["tas"][4]) == (8, 2.1, 114.2578125, 438.0, 0.125, 424)
    assert (m["commb_format"][5], float(f["heading"][5]), m["ias"][5], round(float(f["mach"][5]), 3), m["baro_rate"][5]) == \
           (9, 42.71484375, 252, 0.42, -1920)
    assert (m["commb_format"][6], m["nav_mcp_altitude"][6], m["nav_fms_altitude"][6]) == (7, 3008, 3008)
    assert f["nav_qnh"][6] == np.float32(1020.0)
    assert m["nav_mcp_altitude"][7] == 16992 and abs(f["nav_qnh"][7] - 1012.8) < 0.01 and abs(f["nav_heading"][7] - 66.8) < 0.1
