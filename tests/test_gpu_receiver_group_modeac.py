"""Mode A/C per receiver in receiver groups (msd_group_set_receiver_mode_ac, ReceiverGroup.set_receiver_mode_ac).
Every receiver is compared with an oracle that runs Mode A/C exactly when the receiver had it on for that buffer, fed
that receiver's buffers one mag_buf at a time with the FIFO's overlap rule (no end-of-file buffer: a live receiver
never ends).  Each case also checks that Mode A/C replies were actually decoded."""
import numpy as np
import pytest

from helpers import FIELDS, assert_same_stats, fmt_ids

CHUNK = 131072
OVERLAP = 326
pytestmark = pytest.mark.gpu
FMTS = ["uc8", "sc16", "sc16q11"]
STAGES = [0, "host_resolve"]


class AcOracleReceiver:
    """One live receiver in the oracle (fifo.c:176-184, sdr_rtlsdr.c:281-300, sdr_ifile.c:190), as OracleReceiver of
    test_gpu_receiver_group.py, with Mode A/C switchable between buffers: two oracles are fed every buffer, one with
    Mode A/C on and one with it off.  Mode A/C changes nothing of the Mode S path, so either one's Mode S output and
    counters are the receiver's; a buffer's Mode A/C replies come from the first when the switch was on."""

    def __init__(self, oracle, fmt, nfix=1, threshold=58):
        self.on_orc = oracle.Oracle(fmt, threshold, nfix, 1)
        self.off_orc = oracle.Oracle(fmt, threshold, nfix, 0)
        self.counter = 0
        self.carry = None
        self.modeac = 0  # replies of the buffers fed with the switch on

    def feed(self, buf, dropped=0, mode_ac=1):
        self.counter += dropped
        mag, level, power = self.off_orc.convert(buf, CHUNK)
        front = self.carry if (self.carry is not None and dropped == 0) else np.zeros(OVERLAP, np.uint16)
        data = np.concatenate([front, mag])
        ts = int(self.counter * 12e6 / 2400000.0)
        on = self.on_orc.demod_buffer(data, ts, ts // 12000, level, power, cap=1 << 14)
        off = self.off_orc.demod_buffer(data, ts, ts // 12000, level, power, cap=1 << 14)
        ms = on[on["msgtype"] != 32]
        same(ms, off, "Mode S with and without Mode A/C")
        self.carry = data[data.size - OVERLAP:].copy()
        self.counter += CHUNK
        if mode_ac:
            self.modeac += int((on["msgtype"] == 32).sum())
            return on
        return off

    def stats(self):
        st = dict(self.off_orc.stats())
        assert st["demod_modeac"] == 0
        st["demod_modeac"] = self.modeac
        return st


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)
    assert np.array_equal(got["msg"], want["msg"]), what


def stats_equal(gs, ws, dropped=0):
    assert_same_stats(gs, ws)
    assert gs["samples_dropped"] == dropped


def bps(fmt):
    return 2 if fmt == "uc8" else 4


def capture(pkg, fmt_name, seed, nbuf, rate=3000, ac_rate=3000, n_aircraft=12):
    fmt = {"uc8": pkg.siggen.UC8, "sc16": pkg.siggen.SC16, "sc16q11": pkg.siggen.SC16Q11}[fmt_name]
    return pkg.siggen.generate(pkg.siggen.make_cfg(seed=seed, fmt=fmt, msgs_per_sec=rate, ac_per_sec=ac_rate,
                                                   n_aircraft=n_aircraft), nbuf * CHUNK)


def buf_of(iq, k, b):
    return iq[k * CHUNK * b:(k + 1) * CHUNK * b]


def group_flags(pkg, stage):
    return pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0


def run_call(group, refs, entries, on):
    """entries: [(receiver, iq buffer, dropped)]; on: {receiver: switch for this call}.  Sets the switches, submits,
    checks every receiver's messages (Mode S first, then Mode A/C, per buffer) and returns how many Mode A/C replies the
    call delivered."""
    for r, v in on.items():
        group.set_receiver_mode_ac(r, v)
    iq = np.concatenate([e[1] for e in entries])
    got = group.submit(iq, [e[0] for e in entries], [e[2] for e in entries])
    rank = {e[0]: i for i, e in enumerate(entries)}
    assert all(rank[a] <= rank[c] for a, c in zip(got["receiver"][:-1], got["receiver"][1:])), "entry order"
    n_ac = 0
    for r, buf, drop in entries:
        mine = got["m"][got["receiver"] == r]
        want = refs[r].feed(buf, drop, group.receiver_mode_ac(r))
        same(mine, want, f"receiver {r}")
        t = mine["msgtype"] == 32
        assert not t.any() or t[int(np.argmax(t)):].all(), "Mode A/C after Mode S"
        n_ac += int(t.sum())
    return n_ac


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_half_on(pkg, oracle, fmt, stage):
    """K = 8, the even receivers with Mode A/C on, 16 calls, the entry order rotated every call."""
    K, calls = 8, 16
    f, of = fmt_ids(pkg, oracle, fmt)
    b = bps(fmt)
    caps = [capture(pkg, fmt, 2100 + 11 * r, calls) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=f, flags=group_flags(pkg, stage))
    refs = [AcOracleReceiver(oracle, of) for _ in range(K)]
    on = {r: int(r % 2 == 0) for r in range(K)}
    n_ac = 0
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        n_ac += run_call(g, refs, [(r, buf_of(caps[r], c, b), 0) for r in order], on if c == 0 else {})
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())
        assert (g.stats(r)["demod_modeac"] > 0) == (r % 2 == 0)
    assert n_ac > 100


def ac_envelope_mag(code12, amp):
    """A Mode A/C reply as 2.4 MHz magnitudes (tests/indep_signal.py's 12 MHz envelope, five ticks a sample)."""
    import indep_signal
    env = indep_signal.mode_ac_envelope(code12)
    env = np.concatenate([env, np.zeros((-env.size) % 5, np.float32)])
    return env.reshape(-1, 5).mean(axis=1) * amp


def ac_stream(nb, places, seed):
    """UC8 stream of nb buffers: a quiet floor and a reply (code, amplitude 0..1) at each of `places` [(sample, code)]."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.0, 0.02, size=nb * CHUNK)
    for s, code in places:
        m = ac_envelope_mag(code, 0.8)
        mag[s:s + m.size] += m
    v = (128 + np.round(np.minimum(mag, 1.0) * 100.0)).astype(np.uint8)
    return np.repeat(v, 2)


@pytest.mark.parametrize("stage", STAGES)
def test_look_behind(pkg, oracle, stage):
    """Replies whose F1 lies in the last 326 samples of a receiver's buffer are decoded in its next buffer, from the
    receiver's own tail; the batch neighbour, another receiver, has a reply at the same place with another code.  After
    dropped > 0 and after reset_receiver the look-behind is zeros."""
    K, nb = 4, 6
    offsets = [CHUNK - 300, CHUNK - 200, CHUNK - 120]
    streams = []
    for r in range(K):
        places = [(k * CHUNK + offsets[k % 3], (0o1200 + 0o111 * r + k) & 0o7777) for k in range(nb - 1)]
        places += [(k * CHUNK + 5000 + 977 * r, 0o7700 - r) for k in range(nb)]
        streams.append(ac_stream(nb, places, 40 + r))
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    refs = [AcOracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    drops = {(2, 3): 4096}
    rng = np.random.default_rng(5)
    n_ac = 0
    for c in range(nb):
        if c == 4:
            g.reset_receiver(1)
            refs[1] = AcOracleReceiver(oracle, oracle.FMT_UC8)
        entries = [(int(r), buf_of(streams[r], c, 2), drops.get((int(r), c), 0)) for r in rng.permutation(K)]
        n_ac += run_call(g, refs, entries, {r: 1 for r in range(K)} if c == 0 else {})
    assert g.receiver_mode_ac(1) == 1  # reset_receiver keeps the switch
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats(), 4096 if r == 2 else 0)
    assert n_ac >= 2 * K * nb - K - 2  # the boundary replies too, but for the drop and the reset


@pytest.mark.parametrize("stage", STAGES)
def test_switching_at_run_time(pkg, oracle, stage):
    K, calls = 6, 10
    caps = [capture(pkg, "uc8", 2600 + r, calls) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    refs = [AcOracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    rng = np.random.default_rng(17)
    n_ac = 0
    for c in range(calls):
        on = {r: int(rng.integers(0, 2)) for r in range(K)}
        entries = [(int(r), buf_of(caps[r], c, 2), 0) for r in rng.permutation(K)]
        n_ac += run_call(g, refs, entries, on)
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())
    assert n_ac > 50


def test_with_receiver_options(pkg, oracle):
    """Mode A/C beside per-receiver thresholds and repair levels."""
    K, calls = 6, 6
    caps = [capture(pkg, "sc16", 2800 + r, calls) for r in range(K)]
    opts = [(58, 1), (40, 2), (75, 0), (58, 2), (90, 1), (30, 0)]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_SC16)
    refs = []
    for r, (thr, nfix) in enumerate(opts):
        g.set_receiver_options(r, preamble_threshold=thr, nfix_crc=nfix)
        refs.append(AcOracleReceiver(oracle, oracle.FMT_SC16, nfix, thr))
    n_ac = 0
    for c in range(calls):
        entries = [((c + k) % K, buf_of(caps[(c + k) % K], c, 4), 0) for k in range(K)]
        n_ac += run_call(g, refs, entries, {r: int((r + c) % 3 != 0) for r in range(K)})
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())
    assert n_ac > 50


@pytest.mark.parametrize("stage", STAGES)
def test_all_off_is_untouched(pkg, oracle, torch_cuda, stage):
    """A group whose switches were set and cleared again delivers the bytes and counters of a group never switched;
    device and host submits deliver the same bytes, with Mode A/C on as well."""
    K, calls = 5, 4
    caps = [capture(pkg, "uc8", 3000 + r, calls) for r in range(K)]
    flags = group_flags(pkg, stage)
    plain = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    toggled = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    dev = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    for r in range(K):
        toggled.set_receiver_mode_ac(r, 1)
        toggled.set_receiver_mode_ac(r, 0)
        assert toggled.receiver_mode_ac(r) == 0
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        host = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        a = plain.submit(host, order)
        b = toggled.submit(host, order)
        assert a.tobytes() == b.tobytes() and not (a["m"]["msgtype"] == 32).any()
    for r in range(K):
        assert plain.stats(r) == toggled.stats(r)
    # host and device submits with Mode A/C on for some receivers
    refs = [AcOracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    n_ac = 0
    for r in range(K):
        dev.set_receiver_mode_ac(r, r % 2)
    for c in range(calls):  # the device group starts at the same buffers as the toggled one did
        order = [(c + k) % K for k in range(K)]
        host = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        got_d = dev.submit(torch_cuda.from_numpy(host).cuda() + 0, order)
        for r in order:
            mine = got_d["m"][got_d["receiver"] == r]
            same(mine, refs[r].feed(buf_of(caps[r], c, 2), 0, r % 2), f"call {c} receiver {r}")
            n_ac += int((mine["msgtype"] == 32).sum())
    gh = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    for r in range(K):
        gh.set_receiver_mode_ac(r, r % 2)
    dev2 = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=flags)
    for r in range(K):
        dev2.set_receiver_mode_ac(r, r % 2)
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        host = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        assert gh.submit(host, order).tobytes() == dev2.submit(torch_cuda.from_numpy(host).cuda() + 0, order).tobytes()
    for r in range(K):
        stats_equal(dev.stats(r), refs[r].stats())
        assert gh.stats(r) == dev.stats(r)
    assert n_ac > 20


def test_overflow_rescan(pkg, oracle):
    """A receiver of full-scale noise among quiet ones overflows the region slices at this arena size; the call is
    scanned again in pieces with Mode A/C on for half of the receivers, the noisy one included."""
    K = 64
    rng = np.random.default_rng(9)
    quiet = [capture(pkg, "uc8", 3300 + r, 2, rate=500, ac_rate=3000) for r in range(K)]
    loud = rng.integers(0, 256, size=2 * CHUNK * 2, dtype=np.uint8)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, test_arena_permille=40)
    refs = [AcOracleReceiver(oracle, oracle.FMT_UC8) for _ in range(K)]
    src = [loud if r == 3 else quiet[r] for r in range(K)]
    n_ac = 0
    for c in range(2):
        n_ac += run_call(g, refs, [(r, buf_of(src[r], c, 2), 0) for r in range(K)],
                         {r: int(r % 2 == 1) for r in range(K)} if c == 0 else {})
    assert g.timing()["reruns"] > 0
    for r in range(K):
        stats_equal(g.stats(r), refs[r].stats())
    assert n_ac > 100


def test_size_1024(pkg, oracle):
    K = 1024
    base = capture(pkg, "uc8", 4343, 64, rate=3000, ac_rate=2000)
    iq = np.empty(K * CHUNK * 2, dtype=np.uint8)
    for r in range(K):
        iq[r * CHUNK * 2:(r + 1) * CHUNK * 2] = buf_of(base, (r * 7) % 64, 2)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8)
    on = [int(r % 3 != 1) for r in range(K)]  # a spread: two in three on
    for r in range(K):
        if on[r]:
            g.set_receiver_mode_ac(r, 1)
    got = g.submit(iq, list(range(K)))
    n_ac = 0
    for r in list(range(0, K, 16)) + [1, 4, 1021, 1022, 1023]:
        ref = AcOracleReceiver(oracle, oracle.FMT_UC8)
        mine = got["m"][got["receiver"] == r]
        same(mine, ref.feed(buf_of(iq, r, 2), 0, on[r]), f"receiver {r}")
        stats_equal(g.stats(r), ref.stats())
        n_ac += int((mine["msgtype"] == 32).sum())
    assert n_ac > 100


def test_errors_leave_state_untouched(pkg, oracle):
    capi = pkg.capi
    caps = [capture(pkg, "uc8", 3600 + r, 2) for r in range(3)]
    g = capi.ReceiverGroup(3, fmt=capi.FMT_UC8)
    refs = [AcOracleReceiver(oracle, oracle.FMT_UC8) for _ in range(3)]
    run_call(g, refs, [(r, buf_of(caps[r], 0, 2), 0) for r in range(3)], {1: 1})
    before = [g.stats(r) for r in range(3)]
    L = capi._group_lib()
    for r, v in ((3, 1), (0, 2), (1, -1), (2, 0x100)):
        assert L.msd_group_set_receiver_mode_ac(g._h, r, v) == -22
    with pytest.raises(capi.MsdError, match="-22"):
        g.set_receiver_mode_ac(5, 1)
    with pytest.raises(capi.MsdError, match="-22"):
        g.receiver_mode_ac(3)
    on = capi.C.c_int(7)
    assert L.msd_group_get_receiver_mode_ac(g._h, 3, capi.C.byref(on)) == -22 and on.value == 7
    assert L.msd_group_get_receiver_mode_ac(g._h, 0, None) == -22
    assert L.msd_group_set_receiver_mode_ac(None, 0, 1) == -22
    assert L.msd_group_get_receiver_mode_ac(None, 0, capi.C.byref(on)) == -22
    assert [g.receiver_mode_ac(r) for r in range(3)] == [0, 1, 0]
    assert [g.stats(r) for r in range(3)] == before
    run_call(g, refs, [(r, buf_of(caps[r], 1, 2), 0) for r in range(3)], {})
    for r in range(3):
        stats_equal(g.stats(r), refs[r].stats())
    assert g.stats(1)["demod_modeac"] > 0 and g.stats(0)["demod_modeac"] == 0
    with pytest.raises(capi.MsdError, match="-22"):  # the group-wide flag stays refused
        capi.ReceiverGroup(4, fmt=capi.FMT_UC8, mode_ac=1)
