"""Decoded fields with every receiver's messages in receiver groups (msd_group_submit_device_fields,
msd_group_submit_host_fields; ReceiverGroup.submit(..., fields=True)).  Every delivered fields record is compared with
the host's msd_decode_fields on the delivered message -- a Mode A/C reply with the fields of the previous Mode A/C reply
of the same buffer (one receiver's one entry of one call) as carry, never a neighbour's or an earlier call's -- and, for
Mode S messages, with the oracle's restatement of the field decode.  Every call's messages are also compared with a
second group fed the same buffers through the plain submit: the fields call must not change which messages come out."""
import numpy as np
import pytest

from helpers import FIELDS, assert_same_stats

CHUNK = 131072
OVERLAP = 326
pytestmark = pytest.mark.gpu
STAGES = [0, "host_resolve"]


def group_flags(pkg, stage, fields=True):
    return (pkg.capi.CFG_DECODE_FIELDS if fields else 0) | (pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0)


def bps(fmt):
    return 2 if fmt == "uc8" else 4


def capture(pkg, fmt_name, seed, nbuf, rate=4000, ac_rate=2000, n_aircraft=12):
    fmt = {"uc8": pkg.siggen.UC8, "sc16": pkg.siggen.SC16}[fmt_name]
    return pkg.siggen.generate(pkg.siggen.make_cfg(seed=seed, fmt=fmt, msgs_per_sec=rate, ac_per_sec=ac_rate,
                                                   n_aircraft=n_aircraft), nbuf * CHUNK)


def buf_of(iq, k, b):
    return iq[k * CHUNK * b:(k + 1) * CHUNK * b]


def field_names(pkg):
    return [n for n in pkg.capi.FIELDS_DTYPE.names if n != "pad2"]


def host_fields(pkg, msgs):
    """msd_decode_fields over the messages of ONE buffer, in delivery order: the carry of a Mode A/C reply is the fields
    of the previous Mode A/C reply of this buffer, NULL for its first one and for every Mode S message."""
    out = np.zeros(len(msgs), dtype=pkg.capi.FIELDS_DTYPE)
    carry = None
    for i, m in enumerate(msgs):
        if m["msgtype"] == 32:
            out[i] = pkg.capi.decode_fields(m, carry)
            carry = out[i]
        else:
            out[i] = pkg.capi.decode_fields(m)
    return out


def check_buffer(pkg, oracle, msgs, fields, what):
    """One buffer's delivered records against the host decode and (Mode S) the oracle; Mode S first, then Mode A/C."""
    assert len(msgs) == len(fields), what
    t = msgs["msgtype"] == 32
    assert not t.any() or t[int(np.argmax(t)):].all(), (what, "Mode A/C after Mode S")
    want = host_fields(pkg, msgs)
    names = field_names(pkg)
    for f in names:
        bad = np.flatnonzero(fields[f] != want[f])
        assert bad.size == 0, (what, f, int(bad[0]), fields[f][bad[0]], want[f][bad[0]], int(msgs["msgtype"][bad[0]]))
    assert fields.tobytes() == want.tobytes(), (what, "bytes between the members")
    ms = np.flatnonzero(~t)
    if ms.size:
        orc = np.array([oracle.fields_of(msgs[i]) for i in ms], dtype=fields.dtype)
        for f in names:
            bad = np.flatnonzero(fields[f][ms] != orc[f])
            assert bad.size == 0, (what, "oracle", f, int(ms[bad[0]]), fields[f][ms[bad[0]]], orc[f][bad[0]])


def fields_call(pkg, oracle, group, plain, entries, iq=None, what=""):
    """entries: [(receiver, iq buffer, dropped)].  One fields call on `group` and the same call through the plain submit
    on `plain`; checks order, messages and every fields record; returns {receiver: (messages, fields)}."""
    host = np.concatenate([e[1] for e in entries])
    rx, drops = [e[0] for e in entries], [e[2] for e in entries]
    got, ff = group.submit(host if iq is None else iq, rx, drops, fields=True)
    ref = plain.submit(host, rx, drops)
    assert got.tobytes() == ref.tobytes(), (what, "messages of the fields call and of the plain call")
    assert len(ff) == len(got)
    rank = {r: i for i, r in enumerate(rx)}
    assert all(rank[a] <= rank[c] for a, c in zip(got["receiver"][:-1], got["receiver"][1:])), "entry order"
    out = {}
    for r in rx:
        sel = got["receiver"] == r
        out[r] = (np.ascontiguousarray(got["m"][sel]), np.ascontiguousarray(ff[sel]))
        check_buffer(pkg, oracle, out[r][0], out[r][1], f"{what} receiver {r}")
    return out


class OracleReceiver:
    """One live receiver in the oracle: the FIFO's overlap (fifo.c:176-184), the sample clock of rtlsdrCallback
    (sdr_rtlsdr.c:281-300) and the --ifile system clock (sdr_ifile.c:190); Mode A/C on or off for its whole life."""

    def __init__(self, oracle, fmt, mode_ac):
        self.orc = oracle.Oracle(fmt, 58, 1, mode_ac)
        self.counter = 0
        self.carry = np.zeros(OVERLAP, np.uint16)

    def feed(self, buf):
        mag, level, power = self.orc.convert(buf, CHUNK)
        data = np.concatenate([self.carry, mag])
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


def fmt_id(pkg, fmt):
    return {"uc8": pkg.capi.FMT_UC8, "sc16": pkg.capi.FMT_SC16}[fmt]


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("fmt", ["uc8", "sc16"])
def test_parity(pkg, oracle, fmt, stage):
    """K = 4, three calls, the entry order rotated every call, Mode A/C on for receivers 0 and 2."""
    K, calls = 4, 3
    b = bps(fmt)
    caps = [capture(pkg, fmt, (5100 if fmt == "uc8" else 5200) + r, calls) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=fmt_id(pkg, fmt), flags=group_flags(pkg, stage))
    plain = pkg.capi.ReceiverGroup(K, fmt=fmt_id(pkg, fmt), flags=group_flags(pkg, stage, fields=False))
    for r in (0, 2):
        g.set_receiver_mode_ac(r, 1)
        plain.set_receiver_mode_ac(r, 1)
    decoded = short = n_ac = 0
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        out = fields_call(pkg, oracle, g, plain, [(r, buf_of(caps[r], c, b), 0) for r in order], what=f"call {c}")
        for m, f in out.values():
            df17 = m["msgtype"] == 17
            decoded += int(((f["cpr_valid"] != 0) | (f["callsign_valid"] != 0) | (f["velocity_valid"] != 0))[df17].sum())
            short += int((m["msgbits"] == 56).sum())
            n_ac += int((m["msgtype"] == 32).sum())
    assert decoded > 0 and short > 0 and n_ac > 0, (decoded, short, n_ac)
    for r in range(K):
        assert g.stats(r) == plain.stats(r)
    assert g.timing()["resolve_passes"] == (0 if stage == "host_resolve" else 1)


@pytest.mark.parametrize("stage", STAGES)
def test_against_a_context_of_its_own(pkg, oracle, torch_cuda, stage):
    """Receiver 1 of a K = 3 group against a Demodulator with CFG_DECODE_FIELDS fed the same buffers with launch_device
    without `last`, then collect_fields: messages and fields byte-identical."""
    K, calls = 3, 3
    caps = [capture(pkg, "uc8", 5300 + r, calls) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    plain = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage, fields=False))
    g.set_receiver_mode_ac(1, 1)
    plain.set_receiver_mode_ac(1, 1)
    dem = pkg.capi.Demodulator(fmt=pkg.capi.FMT_UC8, mode_ac=1, decode_fields=True,
                               flags=pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0)
    n = n_ac = 0
    for c in range(calls):
        order = [(c + k) % K for k in range(K)]
        host = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        dev = torch_cuda.from_numpy(host).cuda()
        out = fields_call(pkg, oracle, g, plain, [(r, buf_of(caps[r], c, 2), 0) for r in order], iq=dev, what=f"call {c}")
        own = torch_cuda.from_numpy(np.ascontiguousarray(buf_of(caps[1], c, 2))).cuda()
        dem.launch_device(own.data_ptr(), CHUNK, last=False)
        wm, wf = dem.collect_fields()
        gm, gf = out[1]
        assert gm.tobytes() == wm.tobytes(), f"call {c}: messages"
        assert gf.tobytes() == wf.tobytes(), f"call {c}: fields"
        n += len(gm)
        n_ac += int((gm["msgtype"] == 32).sum())
    assert n > 100 and n_ac > 0


def mode_a_to_code12(mode_a):
    """A Mode A code in the hex-digit form of msd_message.msg (A4 A2 A1 = 0x4000 0x2000 0x1000, B = 0x0400.., C = 0x0040..,
    D = 0x0004..) as the twelve pulses in the order they are sent: C1 A1 C2 A2 C4 A4 (X) B1 D1 B2 D2 B4 D4."""
    order = [0x0010, 0x1000, 0x0020, 0x2000, 0x0040, 0x4000, 0x0100, 0x0001, 0x0200, 0x0002, 0x0400, 0x0004]
    code = 0
    for bit in order:
        code = (code << 1) | (1 if mode_a & bit else 0)
    return code


def ac_envelope_mag(code12, amp):
    """A Mode A/C reply as 2.4 MHz magnitudes (tests/indep_signal.py's 12 MHz envelope, five ticks a sample)."""
    import indep_signal
    env = indep_signal.mode_ac_envelope(code12)
    env = np.concatenate([env, np.zeros((-env.size) % 5, np.float32)])
    return env.reshape(-1, 5).mean(axis=1) * amp


def ac_stream(nb, places, seed):
    """UC8 stream of nb buffers: a quiet floor and a reply (Mode A code, hex-digit form) at each of `places`
    [(sample, mode_a)]."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.0, 0.02, size=nb * CHUNK)
    for s, mode_a in places:
        m = ac_envelope_mag(mode_a_to_code12(mode_a), 0.8)
        mag[s:s + m.size] += m
    v = (128 + np.round(np.minimum(mag, 1.0) * 100.0)).astype(np.uint8)
    return np.repeat(v, 2)


ALT_100, ALT_0, NOT_ALT, NOT_ALT_2 = 0x0630, 0x0620, 0x7777, 0x5555  # (tests/test_fields.py: 0x0630 is 100 ft, 0x0620 0 ft)
# receiver A: an altitude code, then codes that are none (they inherit), another altitude, one more that inherits; its
# second buffer begins with a code that is no altitude.  Receiver B, behind A in every call, begins with one too.
CARRY_A = [(3000, ALT_100), (9000, NOT_ALT), (15000, NOT_ALT_2), (40000, ALT_0), (46000, NOT_ALT),
           (CHUNK + 3000, NOT_ALT), (CHUNK + 9000, ALT_0), (CHUNK + 15000, NOT_ALT_2)]
CARRY_B = [(2500, NOT_ALT), (8000, NOT_ALT_2), (20000, ALT_100), (26000, NOT_ALT),
           (CHUNK + 2500, NOT_ALT_2), (CHUNK + 30000, ALT_0)]
CARRY_C = [(5000, ALT_0), (CHUNK + 5000, ALT_100), (CHUNK + 11000, NOT_ALT)]


@pytest.mark.parametrize("stage", STAGES)
def test_mode_ac_carry_stays_inside_a_buffer(pkg, oracle, stage):
    streams = [ac_stream(2, CARRY_A, 71), ac_stream(2, CARRY_B, 72), ac_stream(2, CARRY_C, 73)]
    g = pkg.capi.ReceiverGroup(3, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    plain = pkg.capi.ReceiverGroup(3, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage, fields=False))
    for r in range(3):
        g.set_receiver_mode_ac(r, 1)
        plain.set_receiver_mode_ac(r, 1)
    outs = [fields_call(pkg, oracle, g, plain, [(r, buf_of(streams[r], c, 2), 0) for r in (2, 0, 1)], what=f"call {c}")
            for c in range(2)]

    def replies(c, r):
        m, f = outs[c][r]
        sel = m["msgtype"] == 32
        return (m["msg"][sel, 0].astype(int) << 8 | m["msg"][sel, 1]).tolist(), f[sel]

    for c, r, places in ((0, 0, CARRY_A[:5]), (1, 0, CARRY_A[5:]), (0, 1, CARRY_B[:4]), (1, 1, CARRY_B[4:])):
        codes, _ = replies(c, r)
        assert codes == [p[1] for p in places], (c, r, [hex(x) for x in codes])
    codes, fa = replies(0, 0)
    own = [pkg.capi.decode_fields(m)["altitude_baro_valid"] for m in outs[0][0][0][outs[0][0][0]["msgtype"] == 32]]
    assert own == [1, 0, 0, 1, 0]
    assert fa["altitude_baro_valid"].tolist() == [1, 1, 1, 1, 1]  # the second, third and fifth inherited theirs
    assert fa["altitude_baro"].tolist() == [100, 100, 100, 0, 0]
    assert fa["squawk"].tolist() == [ALT_100, NOT_ALT, NOT_ALT_2, ALT_0, NOT_ALT]
    # B is A's neighbour behind it in the batch, and A's first buffer ended on a carried altitude
    _, fb = replies(0, 1)
    assert fb["altitude_baro_valid"].tolist() == [0, 0, 1, 1]
    _, fa2 = replies(1, 0)
    assert fa2["altitude_baro_valid"].tolist() == [0, 1, 1]
    _, fb2 = replies(1, 1)
    assert fb2["altitude_baro_valid"].tolist() == [0, 1]
    assert g.timing()["resolve_passes"] == (0 if stage == "host_resolve" else 1)


def test_rescanned_call(pkg, oracle):
    """A receiver of full-scale noise among quiet ones overflows the region slices at this arena size (K = 64: the
    arenas are at their floor of one hit per position of one buffer, 32 hits per 2048-position tile, which
    test_gpu_receiver_group.py::test_overflow_rescan shows noise to exceed; fewer receivers have more room per tile);
    the call is scanned again in pieces and every entry resolved on the host."""
    K = 64
    rng = np.random.default_rng(9)
    quiet = [capture(pkg, "uc8", 5500 + r, 2, rate=500, ac_rate=3000) for r in range(K)]
    loud = rng.integers(0, 256, size=2 * CHUNK * 2, dtype=np.uint8)
    src = [loud if r == 3 else quiet[r] for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, 0), test_arena_permille=40)
    plain = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, test_arena_permille=40)
    for r in range(1, K, 2):
        g.set_receiver_mode_ac(r, 1)
        plain.set_receiver_mode_ac(r, 1)
    n = n_ac = 0
    assert g.timing()["reruns"] == 0
    for c in range(2):
        out = fields_call(pkg, oracle, g, plain, [(r, buf_of(src[r], c, 2), 0) for r in range(K)], what=f"call {c}")
        n += sum(len(m) for m, _ in out.values())
        n_ac += sum(int((m["msgtype"] == 32).sum()) for m, _ in out.values())
    t = g.timing()
    assert t["reruns"] > 0 and t["resolve_fallback"] >= K * t["reruns"]  # every entry of a rescanned call on the host
    assert n > 100 and n_ac > 100


def test_group_without_the_flag(pkg, oracle):
    """-EINVAL from both fields entries, and the group decodes its next plain call as one never asked."""
    capi = pkg.capi
    caps = [capture(pkg, "uc8", 5600 + r, 2) for r in range(3)]
    g = capi.ReceiverGroup(3, fmt=capi.FMT_UC8)
    twin = capi.ReceiverGroup(3, fmt=capi.FMT_UC8)
    call = lambda c: np.concatenate([buf_of(caps[r], c, 2) for r in range(3)])
    assert g.submit(call(0), [0, 1, 2]).tobytes() == twin.submit(call(0), [0, 1, 2]).tobytes()
    before = [g.stats(r) for r in range(3)]
    with pytest.raises(capi.MsdError, match="MSD_CFG_DECODE_FIELDS.*-22"):
        g.submit(call(1), [0, 1, 2], fields=True)
    L = capi._group_lib()
    entries = (capi.GroupEntry * 3)(*[capi.GroupEntry(r, 0, 0) for r in range(3)])
    iq = call(1)
    assert L.msd_group_submit_host_fields(g._h, iq.ctypes.data, entries, 3, None, None) == -22
    assert L.msd_group_submit_device_fields(g._h, None, entries, 3, None, None) == -22
    assert L.msd_group_submit_device_fields(None, None, entries, 3, None, None) == -22
    assert [g.stats(r) for r in range(3)] == before
    got = g.submit(call(1), [0, 1, 2])
    assert len(got) > 100 and got.tobytes() == twin.submit(call(1), [0, 1, 2]).tobytes()
    for r in range(3):
        assert g.stats(r) == twin.stats(r)


@pytest.mark.parametrize("stage", STAGES)
def test_plain_and_fields_calls_alternate(pkg, oracle, stage):
    """A group with the flag alternates plain and fields calls; its receivers match oracle receivers throughout, and the
    counters at the end."""
    K, calls = 3, 4
    caps = [capture(pkg, "uc8", 5700 + r, calls) for r in range(K)]
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage))
    plain = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, flags=group_flags(pkg, stage, fields=False))
    on = [1, 0, 1]
    refs = [OracleReceiver(oracle, oracle.FMT_UC8, on[r]) for r in range(K)]
    for r in range(K):
        g.set_receiver_mode_ac(r, on[r])
        plain.set_receiver_mode_ac(r, on[r])
    for c in range(calls):
        order = [(2 * c + k) % K for k in range(K)]
        entries = [(r, buf_of(caps[r], c, 2), 0) for r in order]
        if c % 2:
            out = fields_call(pkg, oracle, g, plain, entries, what=f"call {c}")
            mine = {r: out[r][0] for r in order}
        else:
            host = np.concatenate([e[1] for e in entries])
            mine = g.submit(host, order, as_dict=True)
            ref = plain.submit(host, order, as_dict=True)
            assert all(mine[r].tobytes() == ref[r].tobytes() for r in order), f"call {c}"
        for r in order:
            same(mine[r], refs[r].feed(buf_of(caps[r], c, 2)), f"call {c} receiver {r}")
    for r in range(K):
        assert_same_stats(g.stats(r), refs[r].stats())
        assert g.stats(r) == plain.stats(r)


def test_bad_entries(pkg, oracle):
    """A receiver given twice or out of range: -EINVAL as for submit, the state untouched."""
    capi = pkg.capi
    caps = [capture(pkg, "uc8", 5800 + r, 2) for r in range(3)]
    g = capi.ReceiverGroup(3, fmt=capi.FMT_UC8, flags=capi.CFG_DECODE_FIELDS)
    plain = capi.ReceiverGroup(3, fmt=capi.FMT_UC8)
    fields_call(pkg, oracle, g, plain, [(r, buf_of(caps[r], 0, 2), 0) for r in range(3)], what="call 0")
    before = [g.stats(r) for r in range(3)]
    iq = np.concatenate([buf_of(caps[r], 1, 2) for r in range(3)])
    for bad in ([0, 0, 1], [0, 1, 3], [0, 1, 2, 1]):
        with pytest.raises(capi.MsdError, match="-22"):
            g.submit(np.concatenate([iq, iq]), bad, fields=True)
    L = capi._group_lib()
    entries = (capi.GroupEntry * 3)(*[capi.GroupEntry(r, 0, 0) for r in range(3)])
    entries[1].flags = 1
    assert L.msd_group_submit_host_fields(g._h, iq.ctypes.data, entries, 3, None, None) == -22
    entries[1].flags = 0
    assert L.msd_group_submit_host_fields(g._h, None, entries, 3, None, None) == -22
    assert L.msd_group_submit_device_fields(g._h, capi.C.c_void_p(8), entries, 3, None, None) == -22  # not 16-byte aligned
    assert [g.stats(r) for r in range(3)] == before
    out = fields_call(pkg, oracle, g, plain, [(r, buf_of(caps[r], 1, 2), 0) for r in range(3)], what="call 1")
    assert sum(len(m) for m, _ in out.values()) > 100
