"""Per-receiver options of receiver groups (msd_group_set_receiver_options, ReceiverGroup.set_receiver_options): each
receiver with its own preamble threshold and CRC repair level decodes exactly as a context of its own started with
those options.  The reference for receiver r is the oracle created with r's threshold and level, fed r's buffers one
mag_buf at a time (no end-of-file buffer: a live receiver never ends)."""
import numpy as np
import pytest

from helpers import FIELDS, assert_same_stats, fmt_ids

CHUNK = 131072
OVERLAP = 326
pytestmark = pytest.mark.gpu

DEFAULT = (58, 1)  # the group's msd_config in these tests unless stated


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


def same_list(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS) and np.array_equal(a["msg"], b["msg"])


FMTS = ["uc8", "sc16", "sc16q11"]
STAGES = [0, "host_resolve"]


def group_flags(pkg, stage):
    return pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0


def bps(fmt):
    return 2 if fmt == "uc8" else 4


def capture(pkg, fmt_name, seed, nbuf, rate=4000, n_aircraft=12, noise=0.02):
    fmt = {"uc8": pkg.siggen.UC8, "sc16": pkg.siggen.SC16, "sc16q11": pkg.siggen.SC16Q11}[fmt_name]
    return pkg.siggen.generate(pkg.siggen.make_cfg(seed=seed, fmt=fmt, msgs_per_sec=rate, n_aircraft=n_aircraft,
                                                   noise_fs=noise), nbuf * CHUNK)


def buf_of(iq, k, b):
    return iq[k * CHUNK * b:(k + 1) * CHUNK * b]


def mixed_options(K, seed):
    """Thresholds 40, 58, 75, 400 and random ones in 40..400 (readsb's clamp, demod_2400.h:29-33); levels 0/1/2 mixed."""
    rng = np.random.default_rng(seed)
    thr = [40, 58, 75, 400] + [int(t) for t in rng.integers(40, 401, size=K - 4)]
    lvl = [int(v) for v in rng.permutation([k % 3 for k in range(K)])]
    return list(zip(thr, lvl))


def run_group(group, refs, calls):
    """calls: list of [(receiver, iq buffer, dropped)]; checks every call's messages per receiver against refs."""
    for ci, entries in enumerate(calls):
        iq = np.concatenate([e[1] for e in entries])
        got = group.submit(iq, [e[0] for e in entries], [e[2] for e in entries])
        rank = {e[0]: i for i, e in enumerate(entries)}
        assert all(rank[a] <= rank[c] for a, c in zip(got["receiver"][:-1], got["receiver"][1:])), "entry order"
        for r, buf, drop in entries:
            same(got["m"][got["receiver"] == r], refs[r].feed(buf, drop), f"call {ci} receiver {r}")


def set_all(group, opts):
    for r, (t, n) in enumerate(opts):
        group.set_receiver_options(r, preamble_threshold=t, nfix_crc=n)
        assert group.receiver_options(r) == {"preamble_threshold": t, "nfix_crc": n}


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_options(pkg, oracle, fmt, stage):
    K, calls = 12, 6
    f, of = fmt_ids(pkg, oracle, fmt)
    b = bps(fmt)
    opts = mixed_options(K, 7 + len(fmt))
    caps = [capture(pkg, fmt, 2000 + 11 * r, calls, noise=(0.02, 0.06)[r % 2]) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=f, preamble_threshold=DEFAULT[0], nfix_crc=DEFAULT[1],
                               flags=group_flags(pkg, stage))
    set_all(g, opts)
    refs = [OracleReceiver(oracle, of, n, t) for t, n in opts]
    run_group(g, refs, [[(r, buf_of(caps[r], c, b), 0) for r in range(K)] for c in range(calls)])
    differs = 0
    for r in range(K):
        assert_same_stats(g.stats(r), refs[r].stats())
        # the options matter: the same buffers at the group's default options decode differently
        dflt = OracleReceiver(oracle, of, DEFAULT[1], DEFAULT[0])
        msgs = np.concatenate([dflt.feed(buf_of(caps[r], c, b)) for c in range(calls)])
        mine = OracleReceiver(oracle, of, opts[r][1], opts[r][0])
        want = np.concatenate([mine.feed(buf_of(caps[r], c, b)) for c in range(calls)])
        if not same_list(msgs, want) or dflt.stats() != mine.stats():
            differs += 1
    assert 3 * differs >= K, differs
    # two of the receivers as contexts of their own with the same options
    for r in (0, 3):
        t, n = opts[r]
        d = pkg.capi.Demodulator(fmt=f, preamble_threshold=t, nfix_crc=n, flags=0)
        got = []
        for c in range(calls):
            d.launch_host(buf_of(caps[r], c, b), CHUNK, last=False)
            got.append(d.collect())
        ref = OracleReceiver(oracle, of, n, t)
        same(np.concatenate(got), np.concatenate([ref.feed(buf_of(caps[r], c, b)) for c in range(calls)]),
             f"Demodulator {r}")
        assert_same_stats(d.stats(), g.stats(r))
        d.close()
    g.close()


@pytest.mark.parametrize("stage", STAGES)
def test_mid_stream_threshold_change(pkg, oracle, stage):
    """Receiver 1's threshold moves between calls; a Demodulator told the same at the same points is the reference.
    The other receivers decode as before."""
    K, calls = 4, 8
    caps = [capture(pkg, "uc8", 2500 + r, calls, noise=0.05) for r in range(K)]
    changes = {2: 40, 4: 150, 6: 58}
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    g.set_receiver_options(3, nfix_crc=2)
    refs = {r: OracleReceiver(oracle, oracle.FMT_UC8, 2 if r == 3 else 1) for r in (0, 2, 3)}
    d = pkg.capi.Demodulator(fmt=pkg.capi.FMT_UC8, flags=0)
    for c in range(calls):
        if c in changes:
            g.set_receiver_options(1, preamble_threshold=changes[c])
            d.set_preamble_threshold(changes[c])
        iq = np.concatenate([buf_of(caps[r], c, 2) for r in range(K)])
        got = g.submit(iq, list(range(K)))
        d.launch_host(buf_of(caps[1], c, 2), CHUNK, last=False)
        same(got["m"][got["receiver"] == 1], d.collect(), f"call {c} receiver 1")
        for r in (0, 2, 3):
            same(got["m"][got["receiver"] == r], refs[r].feed(buf_of(caps[r], c, 2)), f"call {c} receiver {r}")
    assert_same_stats(g.stats(1), d.stats())
    for r in (0, 2, 3):
        assert_same_stats(g.stats(r), refs[r].stats())
    assert g.receiver_options(1) == {"preamble_threshold": 58, "nfix_crc": 1}
    d.close()


@pytest.mark.parametrize("stage", STAGES)
def test_fix2_per_call_and_lazy_tables(pkg, oracle, stage):
    """A --no-fix group with one receiver set to --aggressive before its first buffer: the two-bit tables are made
    then, and calls with that receiver (the FIX2 scan) alternate with calls without it."""
    K, calls = 4, 8
    caps = [capture(pkg, "uc8", 2700 + r, calls, noise=0.06) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, nfix_crc=0, flags=group_flags(pkg, stage))
    g.set_receiver_options(2, nfix_crc=2)
    g.set_receiver_options(1, nfix_crc=1)
    lvl = [0, 1, 2, 0]
    refs = [OracleReceiver(oracle, oracle.FMT_UC8, lvl[r]) for r in range(K)]
    pos = [0] * K
    for c in range(calls):
        ids = list(range(K)) if c % 2 == 0 else [3, 1, 0]
        entries = []
        for r in ids:
            entries.append((r, buf_of(caps[r], pos[r], 2), 0))
            pos[r] += 1
        run_group(g, refs, [entries])
    for r in range(K):
        assert_same_stats(g.stats(r), refs[r].stats())
    assert g.stats(2)["buffers"] == calls // 2


def test_overflow_rescan(pkg, oracle):
    """A full-scale-noise receiver at threshold 40 among quiet receivers with mixed options overflows the region
    slices; the batch is scanned again in pieces, every piece with its buffers' own options."""
    K = 64
    rng = np.random.default_rng(19)
    quiet = [capture(pkg, "uc8", 2900 + r, 2, rate=500) for r in range(K)]
    loud = rng.integers(0, 256, size=2 * CHUNK * 2, dtype=np.uint8)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, test_arena_permille=40)
    opts = mixed_options(K, 23)
    opts[3] = (40, opts[3][1])
    set_all(g, opts)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8, n, t) for t, n in opts]
    src = [loud if r == 3 else quiet[r] for r in range(K)]
    run_group(g, refs, [[(r, buf_of(src[r], c, 2), 0) for r in range(K)] for c in range(2)])
    assert g.timing()["reruns"] > 0
    for r in range(K):
        assert_same_stats(g.stats(r), refs[r].stats())


def test_size_1024(pkg, oracle):
    K = 1024
    base = capture(pkg, "uc8", 4343, 64, rate=3000, noise=0.05)
    iq = np.empty(K * CHUNK * 2, dtype=np.uint8)
    for r in range(K):
        iq[r * CHUNK * 2:(r + 1) * CHUNK * 2] = buf_of(base, (r * 7) % 64, 2)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8)
    opts = [(40 + (r * 37) % 361, (r // 16) % 3) for r in range(K)]
    set_all(g, opts)
    got = g.submit(iq, list(range(K)))
    for r in range(0, K, 16):
        t, n = opts[r]
        ref = OracleReceiver(oracle, oracle.FMT_UC8, n, t)
        same(got["m"][got["receiver"] == r], ref.feed(buf_of(iq, r, 2)), f"receiver {r}")
        assert_same_stats(g.stats(r), ref.stats())


def test_errors_and_defaults(pkg, oracle):
    capi = pkg.capi
    K = 3
    caps = [capture(pkg, "uc8", 3100 + r, 3) for r in range(K)]
    g = capi.ReceiverGroup(K, fmt=capi.FMT_UC8, preamble_threshold=75, nfix_crc=2)
    for r in range(K):  # untouched receivers carry the group's configuration
        assert g.receiver_options(r) == {"preamble_threshold": 75, "nfix_crc": 2}
    g.set_receiver_options(1, preamble_threshold=40, nfix_crc=0)
    refs = [OracleReceiver(oracle, oracle.FMT_UC8, 0 if r == 1 else 2, 40 if r == 1 else 75) for r in range(K)]
    run_group(g, refs, [[(r, buf_of(caps[r], 0, 2), 0) for r in range(K)]])
    before = [(g.stats(r), g.receiver_options(r)) for r in range(K)]
    L = capi._group_lib()

    def raw_set(receiver, thr, nfix, reserved=(0, 0)):
        o = capi.GroupReceiverOptions(thr, nfix, (capi.C.c_int32 * 2)(*reserved))
        return L.msd_group_set_receiver_options(g._h, receiver, capi.C.byref(o))

    assert raw_set(K, 58, 1) == -22
    assert raw_set(0, 0, 2) == -22
    assert raw_set(0, 401, 2) == -22
    assert raw_set(0, 75, 3) == -22
    assert raw_set(0, 75, -1) == -22
    assert raw_set(0, 75, 2, (1, 0)) == -22
    assert raw_set(0, 75, 2, (0, 1)) == -22
    assert L.msd_group_set_receiver_options(g._h, 0, None) == -22
    assert L.msd_group_get_receiver_options(g._h, K, capi.C.byref(capi.GroupReceiverOptions())) == -22
    with pytest.raises(capi.MsdError, match="-22"):
        g.set_receiver_options(0, preamble_threshold=401)
    # the repair level is fixed once a receiver has history; the threshold and the current level are not
    with pytest.raises(capi.MsdError, match="-16"):
        g.set_receiver_options(0, nfix_crc=1)
    assert raw_set(0, 75, 2) == 0
    assert [(g.stats(r), g.receiver_options(r)) for r in range(K)] == before
    # decoding runs on as if nothing had happened
    run_group(g, refs, [[(r, buf_of(caps[r], 1, 2), 0) for r in range(K)]])
    for r in range(K):
        assert_same_stats(g.stats(r), refs[r].stats())
    # a reset keeps the options and frees the level
    g.reset_receiver(1)
    assert g.receiver_options(1) == {"preamble_threshold": 40, "nfix_crc": 0}
    g.set_receiver_options(1, nfix_crc=1)
    g.set_receiver_options(1, nfix_crc=2)
    # the group-wide threshold sets every receiver's
    g.set_preamble_threshold(100)
    assert [g.receiver_options(r) for r in range(K)] == [{"preamble_threshold": 100, "nfix_crc": 2}] * K
    with pytest.raises(capi.MsdError, match="-22"):
        g.set_preamble_threshold(0)
    refs[1] = OracleReceiver(oracle, oracle.FMT_UC8, 2, 100)
    got = g.submit(buf_of(caps[1], 2, 2), [1])
    same(got["m"], refs[1].feed(buf_of(caps[1], 2, 2)), "receiver 1 after its reset")
    assert_same_stats(g.stats(1), refs[1].stats())


@pytest.mark.parametrize("stage", STAGES)
def test_uniform_options_unchanged(pkg, oracle, stage):
    """Receivers set explicitly to the group's own options deliver the bytes an untouched group delivers."""
    K, calls = 6, 4
    caps = [capture(pkg, "uc8", 3300 + r, calls, noise=0.04) for r in range(K)]
    flags = group_flags(pkg, stage)
    plain = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, preamble_threshold=75, nfix_crc=2, flags=flags)
    set_ = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, preamble_threshold=75, nfix_crc=2, flags=flags)
    for r in range(K):
        set_.set_receiver_options(r, preamble_threshold=75, nfix_crc=2)
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        iq = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        a, b = plain.submit(iq, order), set_.submit(iq, order)
        assert len(a) > 0 and a.tobytes() == b.tobytes()
    for r in range(K):
        assert plain.stats(r) == set_.stats(r)
