"""MSD_FMT_MAG16 contexts on the GPU, and the demodulator's exact comparisons reached on purpose: the constructed scenes of
tests/mag_scenes.py through launch_device / launch_host with both resolve stages, against the oracle's MAG16 replay
(messages, counters, noise and signal power bit for bit) and, where the scene has one, against its designed answer."""
import errno

import numpy as np
import pytest

import mag_scenes as ms
from helpers import assert_same, oracle_live_feed

pytestmark = pytest.mark.gpu

C = ms.CHUNK


@pytest.fixture(params=["gpu-resolve", "host-resolve"], autouse=True)
def resolve_stage(request, monkeypatch):
    monkeypatch.setenv("MSD_GPU_RESOLVE", "1" if request.param == "gpu-resolve" else "0")
    return request.param


def to_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")


def run(pkg, torch, mag, thr=58, nfix=1, batch_bufs=4, via="device", dem=None):
    """The capture through the pipelined stream interface in batches of batch_bufs buffers."""
    batch = batch_bufs * C
    n = mag.size
    if dem is None:
        dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, preamble_threshold=thr, nfix_crc=nfix, max_batch_samples=batch,
                              message_capacity=1 << 16)
    if via == "device":
        d = to_device(torch, np.concatenate([mag, np.zeros(32, np.uint16)]))
        return pkg.replay_device(dem, d.data_ptr(), n, batch), dem
    out, inflight, off, keep = [], 0, 0, []
    while True:
        m = min(batch, n - off)
        if inflight == pkg.capi.PIPELINE_DEPTH:
            out.append(dem.collect())
            inflight -= 1
            keep.pop(0)
        part = np.ascontiguousarray(mag[off:off + m]) if m else np.zeros(1, np.uint16)
        keep.append(part)   # alive until collected
        dem.launch_host(part, m, last=off + m >= n)
        inflight += 1
        off += m
        if off >= n:
            break
    while inflight:
        out.append(dem.collect())
        inflight -= 1
    return np.concatenate(out), dem


def oracle_replay(oracle, mag, thr=58, nfix=1, dropped=False):
    orc = oracle.Oracle(oracle.FMT_MAG16, thr, nfix, 0)
    if dropped:
        orc.set_recently_dropped(True)
    return orc.replay(mag, cap=1 << 16, want_means=True)


# ---- a. MAG16 contexts ------------------------------------------------------------------------------------------------

def mag16_capture(pkg, oracle, kind):
    if kind == "random-full-range":
        return np.random.default_rng(9).integers(0, 65536, 6 * C + 1234, dtype=np.uint16)
    n = 8 * C if kind == "exact-multiple" else 7 * C + 4321
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=55, msgs_per_sec=9000, n_aircraft=40), n)
    return oracle.Oracle(oracle.FMT_UC8).convert(iq, n)[0], iq


@pytest.mark.parametrize("via", ["device", "host"])
@pytest.mark.parametrize("batch_bufs", [1, 4, 16])
@pytest.mark.parametrize("kind", ["random-full-range", "siggen", "exact-multiple"])
def test_mag16_context(pkg, oracle, torch_cuda, kind, batch_bufs, via):
    """Magnitudes in: the oracle's MAG16 replay, message for message, counter for counter, the per-buffer means
    (modes_hip.h MSD_FMT_MAG16: from the integer sums) included.  Magnitudes converted from a UC8 capture deliver what the
    UC8 context delivers on that capture."""
    cap = mag16_capture(pkg, oracle, kind)
    mag, iq = (cap, None) if kind == "random-full-range" else cap
    got, dem = run(pkg, torch_cuda, mag, batch_bufs=batch_bufs, via=via)
    want, wstats, wmeans = oracle_replay(oracle, mag)
    assert_same(got, dem.stats(), want, wstats)
    gmeans = dem.buffer_means()
    assert np.array_equal(gmeans, wmeans[-len(gmeans):] if len(gmeans) else gmeans, equal_nan=True)
    if iq is not None:
        assert len(want) > 100
        uc8 = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, max_batch_samples=batch_bufs * C, message_capacity=1 << 16)
        d_iq = torch_cuda.from_numpy(iq).to("cuda:0")   # held until the replay is over
        ugot = pkg.replay_device(uc8, d_iq.data_ptr(), mag.size, batch_bufs * C)
        assert_same(got, dem.stats(), ugot, uc8.stats())
    else:
        assert wstats["demod_preambles"] > 10000


def test_mag16_note_dropped_and_restart(pkg, oracle, torch_cuda):
    """msd_note_dropped in front of the second and third batch (MAGBUF_DISCONTINUOUS: zero look-behind, the clock runs
    on), mirrored by the oracle's live feed; then msd_restart and a second capture on the same context."""
    mag, _ = mag16_capture(pkg, oracle, "siggen")
    cuts, drops = [0, 3 * C, 5 * C, mag.size], [0, 12345, 3 * C + 7]
    segs = [mag[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    want, wstats = oracle_live_feed(oracle.Oracle(oracle.FMT_MAG16, 58, 1, 0), segs, drops)
    d = to_device(torch_cuda, mag)
    dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, nfix_crc=1, max_batch_samples=4 * C, message_capacity=1 << 16)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if drops[i]:
            dem.note_dropped(drops[i])
        dem.launch_device(d.data_ptr() + 2 * a, b - a, last=b == mag.size)
    got = np.concatenate([dem.collect() for _ in range(3)])
    assert len(want) > 100
    assert_same(got, dem.stats(), want, wstats)
    assert dem.stats()["samples_dropped"] == sum(drops)
    # a second capture behind it: a scene with a designed answer
    sc = ms.tie_scene(1, (40,))
    dem.restart()
    got2, _ = run(pkg, torch_cuda, sc.mag, dem=dem)
    want2, wstats2, _ = oracle_replay(oracle, sc.mag)
    ms.check_frames(got2, sc.expected(58)["frames"])
    assert_same(got2, dem.stats(), want2, wstats2)


def test_mag16_with_dc_filter_is_rejected(pkg):
    with pytest.raises(pkg.MsdError, match=str(-errno.EINVAL)):
        pkg.Demodulator(fmt=pkg.FMT_MAG16, dc_filter=True)


# ---- b. preamble tests at equality --------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_bufs", [4, 16])
@pytest.mark.parametrize("thr", [1, 40, 58, 75, 400])
def test_preamble_tests_at_their_bounds(pkg, oracle, torch_cuda, thr, batch_bufs):
    """Each pre-check comparison and each threshold test one below, at and one above its bound, at every residue of the
    scan kernel's 16-position run, the first and last positions of tiles, regions and buffers, mlen - 1, and the short
    last buffer's last position: demod_preambles and demod_preamblePhase as designed."""
    sc = ms.preamble_scene(thr)
    got, dem = run(pkg, torch_cuda, sc.mag, thr=thr, batch_bufs=batch_bufs)
    want, wstats, _ = oracle_replay(oracle, sc.mag, thr)
    assert_same(got, dem.stats(), want, wstats)
    ms.check_counts(dem.stats(), sc.expected(thr))


@pytest.mark.parametrize("thr", [1, 400])
def test_full_scale_base_noise(pkg, oracle, torch_cuda, thr):
    sc = ms.full_scale_scene()
    got, dem = run(pkg, torch_cuda, sc.mag, thr=thr)
    want, wstats, _ = oracle_replay(oracle, sc.mag, thr)
    assert_same(got, dem.stats(), want, wstats)
    ms.check_counts(dem.stats(), sc.expected(thr))


def test_recently_dropped_threshold_at_its_bounds(pkg, oracle, torch_cuda):
    """demod_2400.c:285-290: configured 40, the host's msd_set_preamble_threshold(75) while samples were dropped
    recently; the windows are designed for 75."""
    sc = ms.preamble_scene(75)
    dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, preamble_threshold=40, nfix_crc=1, max_batch_samples=4 * C, message_capacity=1 << 16)
    dem.set_preamble_threshold(75)
    got, _ = run(pkg, torch_cuda, sc.mag, dem=dem)
    want, wstats, _ = oracle_replay(oracle, sc.mag, 40, dropped=True)
    assert_same(got, dem.stats(), want, wstats)
    ms.check_counts(dem.stats(), sc.expected(75))


# ---- c. skip-ahead ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_bufs", [1, 4, 16])
@pytest.mark.parametrize("fate", ["accepted", "bad-crc", "unknown"])
@pytest.mark.parametrize("nbits", [56, 112])
def test_skip_ahead(pkg, oracle, torch_cuda, nbits, fate, batch_bufs):
    """A passing preamble d = msglen * 12 / 5 - 2 .. + 3 positions behind a first frame (formed by the first frame's own
    tail, see mag_scenes.skip_scene): scanned unless the first frame was accepted and d is within its skip
    (demod_2400.c:416)."""
    sc = ms.skip_scene(nbits, fate)
    got, dem = run(pkg, torch_cuda, sc.mag, thr=ms.SKIP_THRESHOLD, nfix=0, batch_bufs=batch_bufs)
    want, wstats, _ = oracle_replay(oracle, sc.mag, ms.SKIP_THRESHOLD, 0)
    assert_same(got, dem.stats(), want, wstats)
    exp = sc.expected(ms.SKIP_THRESHOLD)
    ms.check_frames(got, exp["frames"])
    ms.check_counts(dem.stats(), exp)


# ---- d. buffer and batch edges ------------------------------------------------------------------------------------------

_EDGE = {}


def edge_case(oracle):
    if not _EDGE:
        sc = ms.edge_scene()
        _EDGE["scene"] = sc
        _EDGE["want"] = oracle_replay(oracle, sc.mag)
    return _EDGE["scene"], _EDGE["want"]


@pytest.mark.parametrize("batch_bufs", [1, 4, 16])
def test_frames_at_every_offset_around_a_buffer_boundary(pkg, oracle, torch_cuda, batch_bufs):
    """One frame per buffer, starting at every offset CHUNK - 400 .. CHUNK + 20 of its buffer: read at a buffer's last scan
    positions, straddling into its overlap, or at the next buffer's first ones, inside a batch and across batch
    boundaries; and a frame read at the short last buffer's last position."""
    sc, (want, wstats, _) = edge_case(oracle)
    got, dem = run(pkg, torch_cuda, sc.mag, batch_bufs=batch_bufs)
    assert_same(got, dem.stats(), want, wstats)
    ms.check_frames(got, sc.expected(58)["frames"], rereads=True)


# ---- e. phase ties ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_bufs", [1, 4, 16])
@pytest.mark.parametrize("nfix,flips", ms.TIE_FIXES)
def test_phase_ties_go_to_the_lowest_phase(pkg, oracle, torch_cuda, nfix, flips, batch_bufs):
    """Two or three trial phases of one position slice a frame alike (clean, or with bits --fix / --aggressive correct)
    and score the same: the first-tried, lowest phase wins (bestphase, demod_bestPhase)."""
    sc = ms.tie_scene(nfix, flips)
    got, dem = run(pkg, torch_cuda, sc.mag, nfix=nfix, batch_bufs=batch_bufs)
    want, wstats, _ = oracle_replay(oracle, sc.mag, 58, nfix)
    assert_same(got, dem.stats(), want, wstats)
    exp = sc.expected(58)
    ms.check_frames(got, exp["frames"])
    ms.check_counts(dem.stats(), exp)
    assert dem.stats()["demod_bestPhase"] == [int((got["bestphase"] == p).sum()) for p in range(4, 9)]


# ---- f. ICAO filter order inside a batch --------------------------------------------------------------------------------

@pytest.mark.parametrize("nfix", [1, 2])
@pytest.mark.parametrize("batch_bufs", [4, 8])
def test_filter_order_inside_a_batch(pkg, oracle, torch_cuda, batch_bufs, nfix):
    """A fresh context: AP formats of A before and after the DF11 that adds it, in its buffer and later ones; DF11 with
    IID 3 of an unknown address; corrected DF17s of unknown addresses; corrected DF11s of a known and of an unknown
    address; the first clean squitter of D hidden by the skip of the DF17 in front of it, then corrected DF17s and an AP
    format of D (for the GPU resolver, a probation-table entry that fails: mag_scenes.filter_scene)."""
    sc = ms.filter_scene()
    got, dem = run(pkg, torch_cuda, sc.mag, nfix=nfix, batch_bufs=batch_bufs)
    want, wstats, _ = oracle_replay(oracle, sc.mag, 58, nfix)
    assert_same(got, dem.stats(), want, wstats)
    exp = sc.expected(58)
    ms.check_frames(got, exp["frames"])
    ms.check_counts(dem.stats(), exp)


def test_filter_flip_between_two_buffers_of_a_batch(pkg, oracle, torch_cuda):
    """note_dropped moves the clock so that the filter's 60 s flips fall between buffers 0 | 1 of the second batch and
    1 | 2 of the third: A, added in the first batch, is forgotten in the middle of the third (icao_filter.c)."""
    sc, drops = ms.flip_scene()
    cuts = [0, 4 * C, 8 * C, sc.n]
    segs = [sc.mag[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    want, wstats = oracle_live_feed(oracle.Oracle(oracle.FMT_MAG16, 58, 1, 0), segs, drops)
    d = to_device(torch_cuda, sc.mag)
    dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, nfix_crc=1, max_batch_samples=4 * C, message_capacity=1 << 12)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if drops[i]:
            dem.note_dropped(drops[i])
        dem.launch_device(d.data_ptr() + 2 * a, b - a, last=b == sc.n)
    got = np.concatenate([dem.collect() for _ in range(3)])
    assert_same(got, dem.stats(), want, wstats)
    assert [bytes(m["msg"][: m["msgbits"] // 8]) for m in got] == [f["bytes"] for f in sc.frames if f["accept"]]
