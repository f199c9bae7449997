"""The constructed Mode A/C scenes of tests/ac_scenes.py on the CPU: the oracle's MAG16 replay with mode_ac = 1 and the
second reading of the reference (tests/indep_demod.py) must both deliver exactly what each scene was designed to hold,
and every scene must reach both sides of the bounds it names.  No product code."""
import numpy as np
import pytest

import ac_scenes as acs
import indep_demod
from test_indep_demod import assert_second_reading_agrees

D, H, U = acs.DELIVERED, acs.HIDDEN, acs.UNSCANNED


def both_readings(oracle, sc, second=True):
    """Oracle and second reading against each other and against the scene's designed answer; returns the oracle's."""
    msgs, st = oracle.Oracle(oracle.FMT_MAG16, 58, 1, 1).replay(sc.mag, cap=1 << 15)
    exp = sc.expected()
    acs.check_replies(msgs, exp)
    assert st["demod_modeac"] == exp["demod_modeac"]
    if second:
        got, gst = indep_demod.Receiver("mag16", 58, 1, True).replay(sc.mag.tobytes())
        assert_second_reading_agrees(got, gst, msgs, st)
    return msgs, st


def outcomes(sc):
    """{designed outcome: count} of a scene's replies (without those that only keep a buffer from being silent)."""
    out = {}
    for r in (r for r in sc.replies if not r.get("fill")):
        out[r["expect"]] = out.get(r["expect"], 0) + 1
    return out


@pytest.mark.parametrize("which", ["f1", "f2"])
def test_pulse_test_at_its_bounds(oracle, which):
    sc = acs.scene("pulse", which)
    both_readings(oracle, sc)
    reps = 32 if which == "f1" else 1
    cases = acs.pulse_cases(acs.GUESS)
    assert outcomes(sc) == {D: reps * sum(ok is True for _, ok, _ in cases), which: reps * sum(ok is False for _, ok, _ in cases),
                            "noisy": reps}
    assert min(sum(ok is True for _, ok, _ in cases), sum(ok is False for _, ok, _ in cases)) >= 12
    if which == "f1":   # every case at every residue mod 16, in lane 0 and in lane 63 of a tile
        assert {(r["pos"] % acs.TILE) for r in sc.replies} == set(range(16)) | set(range(1008, 1024))
        assert len({(r["pos"] % acs.TILE, r["expect"]) for r in sc.replies}) >= 64
    assert min(sc.noise_levels()[b] for b in sc.used) > 1000   # the level bound is each buffer's own


def test_tile_buffer_and_capture_edges(oracle):
    sc = acs.scene("edge")
    msgs, _ = both_readings(oracle, sc)
    assert outcomes(sc) == {D: len(sc.replies) - 2, U: 2}
    delivered = {(r["b"], r["pos"]) for r in sc.replies if r["expect"] == D}
    assert {(1, 1), (1, acs.CHUNK - 1), (4, 150), (4, 2999), (0, 2 * acs.TILE + 1023), (0, acs.TILE)} <= delivered


def test_clock_of_the_first_pulse(oracle):
    sc = acs.scene("clock")
    both_readings(oracle, sc)
    assert set(outcomes(sc)) == {D} and len(sc.replies) == 2 * (26 + 16) + 4 and outcomes(sc)[D] == 84
    assert sc.clocks == {(base, c) for base in (700, 66000) for c in range(26)}
    assert sc.contracted >= 8   # pairs whose clock a contracted multiply-add would move


def test_bit_windows_at_the_thresholds(oracle):
    sc = acs.scene("window")
    both_readings(oracle, sc)
    assert outcomes(sc) == {D: 19, "noisy": 4, "uncertain": 2, "framing": 2, "quiet": 10}


def test_every_code(oracle):
    sc = acs.scene("codes")
    msgs, _ = both_readings(oracle, sc)
    assert len(msgs) == 8192 and outcomes(sc) == {D: 8192}


def test_skip_ahead(oracle):
    sc = acs.scene("skip")
    both_readings(oracle, sc)
    assert outcomes(sc) == {D: 28, H: 2 + 8, "noisy": 2, "quiet": 1, "f1": 3}


def test_dense_and_loud(oracle):
    sc = acs.scene("dense")
    msgs, st = both_readings(oracle, sc)
    assert sc.levels[:3] == [25364, 0x3fff, 0x4000] and sc.levels[4] == 0
    assert st["demod_modeac"] == 2590 and sum(1 for _, _, b, _ in sc.scanned if b == 0) == 1858


@pytest.mark.parametrize("nb", [57, 113])
def test_many_buffers(oracle, nb):
    """The capture of scene h for a part of 256 CUs (tiles_per_wave 2 and 3): oracle only beyond 57 buffers."""
    sc = acs.scene("waves", nb)
    both_readings(oracle, sc, second=nb <= 57)
    assert outcomes(sc)["f1"] == 2 * nb and outcomes(sc)[D] == len(sc.replies) - 2 * nb
    assert len(set(sc.noise_levels()[:nb])) >= 5


def test_mode_s_beside_it(oracle):
    sc = acs.scene("mixed")
    msgs, _ = both_readings(oracle, sc)
    s = msgs[msgs["msgtype"] != 32]
    want = [f["bytes"] for f in sc.frames if f["accept"]]
    got = [bytes(m["msg"][: m["msgbits"] // 8]) for m in s]
    assert [g for g in got if g != sc.overlapped["bytes"]] == want
    # per buffer: the Mode S messages, then the replies
    kinds = [(int(m["timestampMsg"]) // (5 * acs.CHUNK), m["msgtype"] == 32) for m in msgs]
    assert kinds == sorted(kinds)


def test_builder_refuses_a_wrong_design():
    """finish() fails when a reply does not end as designed, and when a buffer's level is not the designed one."""
    sc = acs.AcScene(acs.CHUNK)
    sc.reply(0, 1000, code=0x0123, extra=(acs.X1,))
    with pytest.raises(AssertionError):
        sc.finish()
    sc = acs.AcScene(acs.CHUNK, {0: 5})
    sc.level(0)
    sc.reply(0, 1000, code=0x0123)
    with pytest.raises(AssertionError, match="another level"):
        sc.finish()
