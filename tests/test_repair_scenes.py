"""The scenes of tests/repair_scenes.py (every one- and two-bit error pattern, once) before any kernel sees them: the
designed answer against the oracle's MAG16 and UC8 replays, against the second reading's score / decode on every frame's
received bytes, and against the second reading's whole demodulator on a thinned scene.  CPU only."""
import numpy as np
import pytest

import indep_demod as D
import mag_scenes as ms
import repair_scenes as rs

SCENES = {"long": rs.long_scene, "short": rs.short_scene}
# accepted per repair level, all blocks; and the DF17 blocks of the long scene alone
ACCEPTED = {"long": (1, 298, 6999), "short": (58, 410, 410)}
ACCEPTED_DF17 = (1, 1 + 107 + 83, 1 + 190 + 6208)


def test_table_counts():
    """The syndromes --fix and --aggressive correct: 107 single bits and 3724 pairs of a 112-bit frame, 51 and all 1275 of
    a 56-bit one; every single bit outside the DF field survives --aggressive's collision passes."""
    for bits, singles, pairs in ((112, rs.SINGLES_112, rs.PAIRS_112), (56, rs.SINGLES_56, rs.PAIRS_56)):
        t1, t2 = D.error_table(bits, 1), D.error_table(bits, 2)
        assert sorted(t1.values()) == [(i,) for i in range(5, bits)] and len(t1) == singles
        assert sum(len(v) == 1 for v in t2.values()) == singles
        assert len(rs.correctable_pairs(bits)) == pairs
        assert all(t2[s] == v for s, v in t1.items())
    assert len(rs.patterns(112)) == 112 + 5671 and len(rs.patterns(56)) == 56 + 1275
    assert len(rs.long_scene().frames) == 1 + 2 * 5783 + 112 + 811
    assert len(rs.short_scene().frames) == 1 + 4 * 1331


@pytest.mark.parametrize("nfix", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_design_counts(name, nfix):
    """What the closed-form rules accept, per level and block."""
    sc = rs.design(SCENES[name](), nfix)
    acc = rs.accepted(sc)
    assert len(acc) == ACCEPTED[name][nfix]
    assert all(f["corrected"] == len(f["pat"]) or name == "short" for f in acc)
    assert not any(f["pat"] and min(f["pat"]) < 5 for f in acc)       # a flipped DF bit is never accepted
    if name == "long":
        assert sum(f["block"] != "A DF18" for f in acc) == ACCEPTED_DF17[nfix]
        per = {b: sum(f["block"] == b for f in acc) for b in ("A DF17", "B DF17", "A DF18")}
        want = {0: (0, 0, 0), 1: (107, 83, 107), 2: (107 + 3724, 83 + 2484, 107 + 493)}[nfix]
        assert (per["A DF17"], per["B DF17"], per["A DF18"]) == want, per
    else:
        plain = [f for f in acc if f["corrected"] == 0]
        fixed = [f for f in acc if f["corrected"] == 1]
        assert len(plain) == 58 and all(f["bytes"] == f["rx"] for f in plain)
        in_place = sum(f["bytes"] == f["clean"] for f in fixed)
        assert (in_place, len(fixed) - in_place) == ((0, 0) if nfix == 0 else (44, 308))
        # the unknown addresses stay unknown, but for the pair that cancels IID 5 and reads as a clean squitter
        assert sum(f["block"].startswith("unknown") for f in acc) == 1


@pytest.mark.parametrize("nfix", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_mag16_replay(oracle, name, nfix):
    sc = rs.design(SCENES[name](), nfix)
    exp = sc.expected(58)
    msgs, st = oracle.Oracle(oracle.FMT_MAG16, 58, nfix, 0).replay(sc.mag, cap=1 << 16)
    ms.check_frames(msgs, exp["frames"])
    ms.check_counts(st, exp)
    assert msgs["correctedbits"].tolist() == [f["corrected"] for f in exp["frames"]]
    assert list(st["demod_accepted"]) == rs.histogram(sc)
    assert len(msgs) == ACCEPTED[name][nfix]


@pytest.mark.parametrize("nfix", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_uc8_replay(oracle, name, nfix):
    """The same frames at one level on the UC8 floor: the designed messages in order, and no more than the cap beyond."""
    sc = rs.design(SCENES[name](), nfix)
    msgs, _ = oracle.Oracle(oracle.FMT_UC8, 58, nfix, 0).replay(rs.to_uc8(sc), cap=1 << 16)
    rs.check_uc8(msgs, sc)


@pytest.mark.parametrize("nfix", [0, 1, 2])
def test_second_reading_scores_and_decodes_every_frame_alike(nfix):
    """indep_demod's scoreModesMessage / decodeModesMessage on the received bytes of every frame, long scene then short
    scene through one filter: the designed verdict, bytes and corrected-bit count."""
    frames = rs.long_scene().frames + rs.short_scene().frames
    rs.design_frames(frames, nfix)
    rx = D.Receiver("mag16", 58, nfix)
    for k, f in enumerate(frames):
        verdict = rx.score(f["rx"], f["msgbits"]) >= 0
        rec = rx.decode(f["rx"])[1] if verdict else None
        assert (rec is not None) == f["accept"], (k, f["block"], f["pat"])
        if rec is not None:
            assert rec["msg"][: f["msgbits"] // 8] == f["bytes"] and rec["correctedbits"] == f["corrected"], (k, f["pat"])
    assert rx.filter.test(rs.A) and not rx.filter.test(rs.B)


THIN = 23


@pytest.mark.parametrize("nfix", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_second_reading_demodulates_a_thinned_scene(oracle, name, nfix):
    """Every 23rd pattern through the whole demodulator of the second reading (plain Python), and through the oracle."""
    sc = rs.design(thin(name), nfix)
    exp = sc.expected(58)
    assert len(exp["frames"]) > (0 if nfix == 0 else 10)
    msgs, st = oracle.Oracle(oracle.FMT_MAG16, 58, nfix, 0).replay(sc.mag, cap=1 << 12)
    ms.check_frames(msgs, exp["frames"])
    ms.check_counts(st, exp)
    got, gst = D.Receiver("mag16", 58, nfix).replay(sc.mag.tobytes())
    ms.check_frames(got, exp["frames"])
    ms.check_counts(gst, exp)
    assert [m["correctedbits"] for m in got] == [f["corrected"] for f in exp["frames"]]
    assert gst["demod_accepted"] == rs.histogram(sc)


_THIN = {}


def thin(name):
    if name not in _THIN:
        _THIN[name] = rs.thinned(SCENES[name](), THIN)
    return _THIN[name]
