"""Receiver groups (msd_group_*, capi.ReceiverGroup): many live receivers decoded in one launch, each exactly as a
context of its own fed the same buffers would decode it -- its own look-behind, clock, ICAO filter and counters.
The reference for every receiver is the oracle fed that receiver's buffers one mag_buf at a time (no end-of-file
buffer: a live receiver never ends)."""
import numpy as np
import pytest

from helpers import FIELDS, assert_same_stats, fmt_ids
import mag_scenes

CHUNK = 131072
OVERLAP = 326
pytestmark = pytest.mark.gpu


class OracleReceiver:
    """One live receiver in the oracle: the FIFO's overlap (fifo.c:176-184), rtlsdrCallback's sample clock over drops
    (sdr_rtlsdr.c:281-300) and the --ifile system clock (sdr_ifile.c:190)."""

    def __init__(self, oracle, fmt, nfix=1, threshold=58):
        self.orc = oracle.Oracle(fmt, threshold, nfix, 0)
        self.counter = 0
        self.carry = None

    def feed(self, buf, dropped=0):
        self.counter += dropped
        mag, level, power = self.orc.convert(buf, CHUNK)
        front = self.carry if (self.carry is not None and dropped == 0) else np.zeros(OVERLAP, np.uint16)
        data = np.concatenate([front, mag])
        ts = int(self.counter * 12e6 / 2400000.0)
        out = self.orc.demod_buffer(data, ts, ts // 12000, level, power, cap=1 << 14)
        self.carry = data[data.size - OVERLAP:].copy()
        self.counter += CHUNK
        return out

    def stats(self):
        return self.orc.stats()


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)
    assert np.array_equal(got["msg"], want["msg"]), what


def stats_equal(gs, ws, dropped=0):
    assert_same_stats(gs, ws)
    assert gs["samples_dropped"] == dropped


FMTS = ["uc8", "sc16", "sc16q11"]


def bps(fmt):
    return 2 if fmt == "uc8" else 4


def capture(pkg, fmt_name, seed, nbuf, rate=4000, n_aircraft=12):
    fmt = {"uc8": pkg.siggen.UC8, "sc16": pkg.siggen.SC16, "sc16q11": pkg.siggen.SC16Q11}[fmt_name]
    return pkg.siggen.generate(pkg.siggen.make_cfg(seed=seed, fmt=fmt, msgs_per_sec=rate, n_aircraft=n_aircraft),
                               nbuf * CHUNK)


def buf_of(iq, k, b):
    return iq[k * CHUNK * b:(k + 1) * CHUNK * b]


def run_group(group, refs, calls, b):
    """calls: list of [(receiver, iq buffer, dropped)]; checks every call's messages per receiver against refs."""
    for ci, entries in enumerate(calls):
        iq = np.concatenate([e[1] for e in entries]) if entries else np.zeros(0, np.uint8)
        got = group.submit(iq, [e[0] for e in entries], [e[2] for e in entries])
        # delivery order: by entry, then stream order
        order = [e[0] for e in entries]
        rank = {r: i for i, r in enumerate(order)}
        assert all(rank[a] <= rank[c] for a, c in zip(got["receiver"][:-1], got["receiver"][1:])), "entry order"
        for r, buf, drop in entries:
            want = refs[r].feed(buf, drop)
            same(got["m"][got["receiver"] == r], want, f"call {ci} receiver {r}")


# flags 0: one pass of the GPU resolve against per-receiver device snapshots; MSD_CFG_HOST_RESOLVE: host threads
STAGES = [0, "host_resolve"]


def group_flags(pkg, stage):
    return pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("nfix", [0, 1, 2])
@pytest.mark.parametrize("fmt", FMTS)
def test_basics(pkg, oracle, fmt, nfix, stage):
    K, calls = 8, 16
    f, of = fmt_ids(pkg, oracle, fmt)
    b = bps(fmt)
    caps = [capture(pkg, fmt, 100 + 7 * r + nfix, calls) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=f, nfix_crc=nfix, flags=group_flags(pkg, stage))
    refs = [OracleReceiver(oracle, of, nfix) for _ in range(K)]
    run_group(g, refs, [[(r, buf_of(caps[r], c, b), 0) for r in range(K)] for c in range(calls)], b)
    total = 0
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())
        total += g.stats(r)["demod_accepted"][0]
    assert total > 100
    # the same receivers as contexts of their own
    for r in (0, K - 1):
        d = pkg.capi.Demodulator(fmt=f, nfix_crc=nfix, flags=0)
        got = []
        for c in range(calls):
            d.launch_host(buf_of(caps[r], c, b), CHUNK, last=False)
            got.append(d.collect())
        ref = OracleReceiver(oracle, of, nfix)
        want = np.concatenate([ref.feed(buf_of(caps[r], c, b)) for c in range(calls)])
        same(np.concatenate(got), want, f"Demodulator {r}")
        stats_equal(d.stats(), g.stats(r))
        d.close()
    g.close()


def uc8_scene(frames):
    """One UC8 buffer holding the given frames [(sample, df, addr)] on a quiet floor (mag_scenes envelopes)."""
    sc = mag_scenes.Scene(CHUNK, seed=len(frames))
    for s, df, addr in frames:
        sc.frame(s, df=df, addr=addr, high=60000)
    v = (128 + np.round(sc.mag.astype(np.float64) * 90.0 / 65535.0)).astype(np.uint8)
    return np.repeat(v, 2)


X = 0x4840D6


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("reverse", [False, True])
def test_isolation(pkg, oracle, stage, reverse):
    """A hears DF17 squitters of X, B only DF4/5/20/21 replies from X: B rejects them as unknown, in either order."""
    squitters = uc8_scene([(1000 + 3000 * k, 17, X) for k in range(30)])
    replies = uc8_scene([(1500 + 3000 * k, (4, 5, 20, 21)[k % 4], X) for k in range(30)])
    g = pkg.capi.ReceiverGroup(2, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(2)]
    calls = []
    for c in range(3):
        e = [(0, squitters, 0), (1, replies, 0)]
        calls.append(e[::-1] if reverse else e)
    run_group(g, refs, calls, 2)
    sa, sb = g.stats(0), g.stats(1)
    stats_equal(sa, refs[0].stats())
    stats_equal(sb, refs[1].stats())
    assert sa["demod_accepted"][0] >= 80
    assert sb["demod_rejected_unknown_icao"] >= 80 and sum(sb["demod_accepted"]) == 0


def test_look_behind(pkg, oracle):
    """A frame at every offset CHUNK-400 .. CHUNK+20 from the start of some buffer of a receiver's stream (one per
    buffer boundary), the entries permuted every call so that the batch neighbour is a different receiver each time."""
    K, rng = 6, np.random.default_rng(3)
    offsets = list(range(CHUNK - 400, CHUNK + 21))
    nb = (len(offsets) + K - 1) // K + 1
    streams = []
    for r in range(K):
        sc = mag_scenes.Scene(nb * CHUNK, seed=r)
        for k, o in enumerate(offsets[r::K]):
            sc.frame(k * CHUNK + o, sub=k % 5, df=(17, 11, 4, 20)[(k + r) % 4], addr=0x100000 + 64 * r + k % 8,
                     high=60000)
        v = (128 + np.round(sc.mag.astype(np.float64) * 90.0 / 65535.0)).astype(np.uint8)
        streams.append(np.repeat(v, 2))
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    calls = [[(int(r), buf_of(streams[r], c, 2), 0) for r in rng.permutation(K)] for c in range(nb)]
    run_group(g, refs, calls, 2)
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())
        assert g.stats(r)["demod_preambles"] >= nb - 2


def test_sparse_participation_and_reset(pkg, oracle):
    M = 16
    ids = [0, 5, 9, 15]
    rng = np.random.default_rng(11)
    caps = {r: capture(pkg, "uc8", 300 + r, 12) for r in ids}
    pos = {r: 0 for r in ids}
    g = pkg.capi.ReceiverGroup(M, fmt=pkg.capi.FMT_UC8)
    refs = {r: OracleReceiver(oracle, oracle.FMT_UC8) for r in ids}
    for c in range(10):
        if c == 5:  # receiver 9 starts over: filter, clock, counters and tail
            g.reset_receiver(9)
            refs[9] = OracleReceiver(oracle, oracle.FMT_UC8)
            before = {r: g.stats(r) for r in ids if r != 9}
        present = [r for r in ids if rng.random() < 0.7]
        entries = []
        for r in rng.permutation(present):
            r = int(r)
            entries.append((r, buf_of(caps[r], pos[r], 2), 0))
            pos[r] += 1
        run_group(g, refs, [entries], 2)
        if c == 5:
            for r, st in before.items():
                if r not in present:
                    assert g.stats(r) == st
    for r in ids:
        stats_equal(g.stats(r), refs[r].stats())
    for r in (1, 2, 14):
        assert g.stats(r)["buffers"] == 0


def test_drops(pkg, oracle):
    K, calls = 4, 8
    caps = [capture(pkg, "uc8", 500 + r, calls) for r in range(K)]
    drops = [[0, 0, 777, 0, 0, 131072 * 3 + 5, 0, 0], [0] * calls, [12345] + [0] * (calls - 1), [0, 1, 0, 1, 0, 1, 0, 1]]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    run_group(g, refs, [[(r, buf_of(caps[r], c, 2), drops[r][c]) for r in range(K)] for c in range(calls)], 2)
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats(), sum(drops[r]))
    # receiver 0 against a Demodulator told about the drops
    d = pkg.capi.Demodulator(fmt=pkg.capi.FMT_UC8, flags=0)
    got = []
    for c in range(calls):
        if drops[0][c]:
            d.note_dropped(drops[0][c])
        d.launch_host(buf_of(caps[0], c, 2), CHUNK, last=False)
        got.append(d.collect())
    ref = OracleReceiver(oracle, oracle.FMT_UC8)
    same(np.concatenate(got), np.concatenate([ref.feed(buf_of(caps[0], c, 2), drops[0][c]) for c in range(calls)]))
    assert d.stats()["samples_dropped"] == g.stats(0)["samples_dropped"]
    d.close()


@pytest.mark.parametrize("stage", STAGES)
def test_filter_flips_on_different_clocks(pkg, oracle, stage):
    """Two receivers whose clocks pass the 60 s flips at different calls (the clocks are moved on by drops: 500 calls
    of 131072 samples are 27.3 s)."""
    calls = 10
    caps = [capture(pkg, "uc8", 700 + r, calls, rate=6000, n_aircraft=6) for r in range(2)]
    gap = 500 * CHUNK
    drops = [[0, gap, gap, 0, gap, gap, 0, gap, 0, 0], [0, 0, 0, gap, gap, 0, gap, gap, gap, gap]]
    g = pkg.capi.ReceiverGroup(2, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(2)]
    run_group(g, refs, [[(r, buf_of(caps[r], c, 2), drops[r][c]) for r in range(2)] for c in range(calls)], 2)
    for r in range(2):
        stats_equal(g.stats(r), refs[r].stats(), sum(drops[r]))
        assert refs[r].counter > 3 * 60 * 2400000 // 2


def test_overflow_rescan(pkg, oracle):
    """A receiver of full-scale noise (preambles everywhere) among quiet ones overflows the region slices (64 buffers:
    32 hits per 2048-position region at this arena size); the batch is scanned again in pieces."""
    K = 64
    rng = np.random.default_rng(9)
    quiet = [capture(pkg, "uc8", 900 + r, 2, rate=500) for r in range(K)]
    loud = rng.integers(0, 256, size=2 * CHUNK * 2, dtype=np.uint8)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, test_arena_permille=40)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    src = [loud if r == 3 else quiet[r] for r in range(K)]
    run_group(g, refs, [[(r, buf_of(src[r], c, 2), 0) for r in range(K)] for c in range(2)], 2)
    assert g.timing()["reruns"] > 0
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())


def test_size_1024(pkg, oracle):
    K = 1024
    base = capture(pkg, "uc8", 4242, 64, rate=3000)
    iq = np.empty(K * CHUNK * 2, dtype=np.uint8)
    for r in range(K):  # 64 distinct buffers, each receiver a different one at a different phase
        iq[r * CHUNK * 2:(r + 1) * CHUNK * 2] = buf_of(base, (r * 7) % 64, 2)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8)
    got = g.submit(iq, list(range(K)))
    for r in range(0, K, 16):
        ref = OracleReceiver(oracle, oracle.FMT_UC8)
        same(got["m"][got["receiver"] == r], ref.feed(buf_of(iq, r, 2)), f"receiver {r}")
        stats_equal(g.stats(r), ref.stats())


def test_errors_leave_state_untouched(pkg, oracle):
    capi = pkg.capi
    caps = [capture(pkg, "uc8", 1200 + r, 3) for r in range(3)]
    g = capi.ReceiverGroup(3, fmt=capi.FMT_UC8)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(3)]
    run_group(g, refs, [[(r, buf_of(caps[r], 0, 2), 0) for r in range(3)]], 2)
    before = [g.stats(r) for r in range(3)]
    two = np.concatenate([buf_of(caps[0], 1, 2), buf_of(caps[1], 1, 2)])
    four = np.concatenate([two, two])
    four = np.concatenate([four, two])
    for iq, rx in ((two, [0, 3]), (two, [1, 1]), (four, [0, 1, 2, 3])):
        with pytest.raises(capi.MsdError, match="-22"):
            g.submit(iq, rx)
    # nonzero flags, and a device pointer that is not 16-byte aligned, straight through the C-ABI
    L = capi._group_lib()
    entries = (capi.GroupEntry * 2)(capi.GroupEntry(0, 0, 0), capi.GroupEntry(1, 1, 0))
    assert L.msd_group_submit_host(g._h, two.ctypes.data, entries, 2, None, None) == -22
    entries[1].flags = 0
    assert L.msd_group_submit_device(g._h, 8, entries, 2, None, None) == -22
    with pytest.raises(capi.MsdError, match="-22"):
        g.reset_receiver(3)
    with pytest.raises(capi.MsdError, match="-22"):
        g.set_preamble_threshold(0)
    assert [g.stats(r) for r in range(3)] == before
    # the look-behind, clocks and filters run on as if nothing had happened
    run_group(g, refs, [[(r, buf_of(caps[r], 1, 2), 0) for r in range(3)]], 2)
    for r in range(3):
        stats_equal(g.stats(r), refs[r].stats())
    for bad in (dict(mode_ac=1), dict(dc_filter=True)):
        with pytest.raises(capi.MsdError, match="-22"):
            capi.ReceiverGroup(4, fmt=capi.FMT_UC8, mode_ac=bad.get("mode_ac", 0),
                               flags=capi.CFG_DC_FILTER if bad.get("dc_filter") else 0)


@pytest.mark.parametrize("stage", STAGES)
def test_device_tensor_matches_host_array(pkg, oracle, torch_cuda, stage):
    """submit() with a ROCm tensor (msd_group_submit_device on the caller's memory, read in place) decodes what the same
    buffers from a numpy array (msd_group_submit_host) decode, call after call."""
    K, calls = 5, 4
    caps = [capture(pkg, "uc8", 1500 + r, calls) for r in range(K)]
    flags = group_flags(pkg, stage)
    gd = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    gh = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        host = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        dev = torch_cuda.from_numpy(host).cuda() + 0  # produced by a torch kernel just before the call
        got_d = gd.submit(dev, order)
        got_h = gh.submit(host, order)
        assert np.array_equal(got_d["receiver"], got_h["receiver"])
        assert got_d.tobytes() == got_h.tobytes()
        for r in order:
            same(got_d["m"][got_d["receiver"] == r], refs[r].feed(buf_of(caps[r], c, 2)), f"call {c} receiver {r}")
    for r in range(K):
        assert gd.stats(r) == gh.stats(r)
        stats_equal(gd.stats(r), refs[r].stats())
    t = gd.timing()
    assert t["hits"] > 0 and t["resolve_passes"] == (0 if stage else 1)
    if not stage:
        assert t["resolve_fallback"] == 0
