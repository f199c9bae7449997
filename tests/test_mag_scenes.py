"""The oracle's MAG16 replay (ORC_FMT_MAG16) on the constructed scenes of tests/mag_scenes.py: it must find exactly what
each scene was designed to hold, and replay magnitudes as it replays the UC8 capture they were converted from.  CPU only."""
import errno

import numpy as np
import pytest

import mag_scenes as ms
from helpers import assert_same, oracle_live_feed


def replay(oracle, mag, thr=58, nfix=1, **kw):
    return oracle.Oracle(oracle.FMT_MAG16, thr, nfix, 0, **kw).replay(mag, cap=1 << 15)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [3 * ms.CHUNK + 4321, 2 * ms.CHUNK, 100])
def test_mag16_replay_of_converted_uc8_equals_uc8_replay(pkg, oracle, n, seed):
    """orc_convert of a UC8 capture, replayed as MAG16: the same messages and counters as the UC8 replay (same per-buffer
    means: both come from the integer sums), including the empty last buffer of an exact multiple."""
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=seed, msgs_per_sec=6000, n_aircraft=30), n)
    want, wstats, wmeans = oracle.Oracle(oracle.FMT_UC8, 58, 1, 0).replay(iq, cap=1 << 15, want_means=True)
    mag = oracle.Oracle(oracle.FMT_UC8, 58, 1, 0).convert(iq, n)[0]
    got, gstats, gmeans = oracle.Oracle(oracle.FMT_MAG16, 58, 1, 0).replay(mag, cap=1 << 15, want_means=True)
    assert_same(got, gstats, want, wstats)
    assert np.array_equal(gmeans, wmeans, equal_nan=True)
    assert n < ms.CHUNK or len(want) > 10


def test_mag16_convert_is_the_identity_with_integer_means(oracle):
    rng = np.random.default_rng(4)
    mag = rng.integers(0, 65536, 5000, dtype=np.uint16)
    out, ml, mp = oracle.Oracle(oracle.FMT_MAG16).convert(mag, mag.size)
    assert np.array_equal(out, mag)
    assert ml == int(mag.astype(np.uint64).sum()) / 65536.0 / mag.size
    assert mp == int((mag.astype(np.uint64) ** 2).sum()) / 65535.0 / 65535.0 / mag.size
    with pytest.raises(ValueError):
        oracle.Oracle(oracle.FMT_MAG16, dc_filter=True)
    orc = oracle.Oracle(oracle.FMT_MAG16)   # the C API rejects it too, as msd_create does
    assert oracle.lib().orc_set_dc_filter(orc._h, 1) == -errno.EINVAL
    assert oracle.lib().orc_set_dc_filter(orc._h, 0) == 0


@pytest.mark.parametrize("thr", [1, 40, 58, 75, 400])
def test_preamble_windows_at_their_bounds(oracle, thr):
    sc = ms.preamble_scene(thr)
    want = sc.expected(thr)
    msgs, st = replay(oracle, sc.mag, thr)
    assert len(msgs) == 0
    ms.check_counts(st, want)
    assert want["demod_preambles"] > len(sc.windows) // 2


@pytest.mark.parametrize("thr", [1, 400])
def test_full_scale_base_noise(oracle, thr):
    sc = ms.full_scale_scene()
    msgs, st = replay(oracle, sc.mag, thr)
    ms.check_counts(st, sc.expected(thr))
    assert (st["demod_preambles"] > 0) == (thr == 1)


def test_recently_dropped_raises_the_threshold(oracle):
    sc = ms.preamble_scene(75)
    orc = oracle.Oracle(oracle.FMT_MAG16, 40, 1, 0)
    orc.set_recently_dropped(True)
    st = orc.replay(sc.mag, cap=1 << 12)[1]
    ms.check_counts(st, sc.expected(75))
    assert sc.expected(75) != sc.expected(40)


@pytest.mark.parametrize("fate", ["accepted", "bad-crc", "unknown"])
@pytest.mark.parametrize("nbits", [56, 112])
def test_skip_ahead(oracle, nbits, fate):
    sc = ms.skip_scene(nbits, fate)
    want = sc.expected(ms.SKIP_THRESHOLD)
    msgs, st = replay(oracle, sc.mag, ms.SKIP_THRESHOLD, 0)
    ms.check_frames(msgs, want["frames"])
    ms.check_counts(st, want)


def test_frames_at_buffer_edges(oracle):
    sc = ms.edge_scene()
    msgs, st = replay(oracle, sc.mag)
    ms.check_frames(msgs, sc.expected(58)["frames"], rereads=True)


@pytest.mark.parametrize("nfix,flips", ms.TIE_FIXES)
def test_phase_ties(oracle, nfix, flips):
    sc = ms.tie_scene(nfix, flips)
    want = sc.expected(58)
    msgs, st = replay(oracle, sc.mag, 58, nfix)
    ms.check_frames(msgs, want["frames"])
    ms.check_counts(st, want)
    assert (msgs["correctedbits"] == len(flips)).all()
    assert sorted(set(msgs["bestphase"].tolist())) == [4, 5, 6, 7, 8]


@pytest.mark.parametrize("nfix", [1, 2])
def test_filter_order(oracle, nfix):
    sc = ms.filter_scene()
    want = sc.expected(58)
    msgs, st = replay(oracle, sc.mag, 58, nfix)
    ms.check_frames(msgs, want["frames"])
    ms.check_counts(st, want)


def test_filter_flip_inside_a_batch(oracle):
    sc, drops = ms.flip_scene()
    C = ms.CHUNK
    segs = [sc.mag[0:4 * C], sc.mag[4 * C:8 * C], sc.mag[8 * C:]]
    msgs, st = oracle_live_feed(oracle.Oracle(oracle.FMT_MAG16, 58, 1, 0), segs, drops)
    assert [int(m["msg"][0]) >> 3 for m in msgs] == [f["df"] for f in sc.frames if f["accept"]]
    assert [bytes(m["msg"][: m["msgbits"] // 8]) for m in msgs] == [f["bytes"] for f in sc.frames if f["accept"]]
