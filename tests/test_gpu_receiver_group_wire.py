"""Wire output per receiver in receiver groups (msd_group_submit_device_wire, msd_group_submit_host_wire): every entry's
bytes against libmsd_host.so's msd_beast_frame_out / msd_avr_line_out applied to the messages an oracle receiver of its
own delivers for that buffer, the message count beside them, and every receiver's counters against its oracle's."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import assert_same_stats
from test_gpu_receiver_group_fields import CHUNK, OVERLAP, buf_of, bps, capture, fmt_id

pytestmark = pytest.mark.gpu
STAGES = [0, "host_resolve"]
K, CALLS = 4, 3
AC_ON = (1, 0, 1, 0)    # Mode A/C on for receivers 0 and 2
NFIX = (1, 1, 1, 2)     # receiver 3 repairs two bits; the group is created at 2
SEEDS = {"uc8": 6100, "sc16": 6200}  # chosen on the CPU: test_parity asserts what they have to contain


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    L.msd_beast_frame_out.restype = C.c_size_t
    L.msd_beast_frame_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.msd_avr_line_out.restype = C.c_size_t
    L.msd_avr_line_out.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


def host_bytes(host, msgs, fmt, verbatim):
    """(bytes, messages forwarded) of the host writers over one entry's messages, in order."""
    msgs = np.ascontiguousarray(msgs)
    buf = (C.c_uint8 * 64)()
    out, n = [], 0
    for i in range(len(msgs)):
        p = msgs[i:i + 1].ctypes.data
        k = host.msd_beast_frame_out(p, int(verbatim), buf) if fmt == 0 else \
            host.msd_avr_line_out(p, int(fmt == 2), int(verbatim), buf)
        out.append(bytes(buf[:k]))
        n += 1 if k else 0
    return b"".join(out), n


class OracleReceiver:
    """One live receiver in the oracle (test_gpu_receiver_group_fields.OracleReceiver with a repair level of its own)."""

    def __init__(self, oracle, fmt, mode_ac, nfix):
        self.orc = oracle.Oracle(fmt, 58, nfix, mode_ac)
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


def parity_captures(pkg, fmt):
    sig = {"uc8": pkg.siggen.UC8, "sc16": pkg.siggen.SC16}[fmt]
    return [pkg.siggen.generate(pkg.siggen.make_cfg(seed=SEEDS[fmt] + r, fmt=sig, msgs_per_sec=4000, ac_per_sec=2000,
                                                    n_aircraft=12, flip_permille=300 if NFIX[r] == 2 else 0),
                                CALLS * CHUNK) for r in range(K)]


_reference = {}


def parity_reference(pkg, oracle, fmt):
    """The captures and, from the oracle group, messages[call][receiver] and the final stats: once per format."""
    if fmt not in _reference:
        caps = parity_captures(pkg, fmt)
        ofmt = {"uc8": oracle.FMT_UC8, "sc16": oracle.FMT_SC16}[fmt]
        refs = [OracleReceiver(oracle, ofmt, AC_ON[r], NFIX[r]) for r in range(K)]
        msgs = [[refs[r].feed(buf_of(caps[r], c, bps(fmt))) for r in range(K)] for c in range(CALLS)]
        _reference[fmt] = (caps, msgs, [refs[r].orc.stats() for r in range(K)])
    return _reference[fmt]


def make_group(pkg, fmt, stage, **kw):
    g = pkg.capi.ReceiverGroup(K, fmt=fmt_id(pkg, fmt), nfix_crc=2,
                               flags=pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0, **kw)
    for r in range(K):
        g.set_receiver_options(r, nfix_crc=NFIX[r])
        g.set_receiver_mode_ac(r, AC_ON[r])
    return g


PARITY = [(f, s, w) for f in ("uc8", "sc16") for s in STAGES for w in ((0, False), (0, True))] + [("uc8", 0, (2, True))]


@pytest.mark.parametrize("fmt,stage,wire", PARITY, ids=lambda v: {(0, False): "beast", (0, True): "beast-verbatim",
                                                                  (2, True): "avr-mlat-verbatim"}.get(v, str(v)))
def test_parity(pkg, oracle, host, torch_cuda, fmt, stage, wire):
    """K = 4, three calls, the entry order rotated every call; host memory in the first two calls, device memory in the
    third.  Beast with and without verbatim for both formats and both resolve stages, the AVR mlat format once."""
    wfmt, verbatim = wire
    caps, want, wstats = parity_reference(pkg, oracle, fmt)
    everything = np.concatenate([m for per_call in want for m in per_call])
    assert (everything["correctedbits"] == 2).sum() >= 1 and (everything["msgtype"] == 32).sum() >= 1
    assert (everything["correctedbits"] == 1).sum() >= 1 and (everything["msgbits"] == 56).sum() >= 1
    g = make_group(pkg, fmt, stage)
    total = 0
    for c in range(CALLS):
        order = [(c + k) % K for k in range(K)]
        iq = np.concatenate([buf_of(caps[r], c, bps(fmt)) for r in order])
        if c == 2:
            got = g.submit_device_wire(torch_cuda.from_numpy(iq).cuda(), order, wfmt, verbatim=verbatim)
        else:
            got = g.submit_host_wire(iq, order, wfmt, verbatim=verbatim)
        assert [e[0] for e in got] == order, f"call {c}: one sink call per entry, in entry order"
        for r, data, nmsgs in got:
            exp, n = host_bytes(host, want[c][r], wfmt, verbatim)
            assert nmsgs == n, (c, r, nmsgs, n, len(want[c][r]))
            assert data == exp, (c, r, len(data), len(exp))
            total += n
    assert total > 100
    for r in range(K):
        assert_same_stats(g.stats(r), wstats[r])
    assert g.timing()["resolve_passes"] == (0 if stage == "host_resolve" else 1)


@pytest.mark.parametrize("stage", STAGES)
def test_mixed_calls(pkg, oracle, host, stage):
    """A group that alternates plain and wire calls against a twin fed the same buffers through the plain call only:
    the same messages in the plain calls, their bytes in the wire calls, the same counters at the end."""
    calls = 4
    caps, _, _ = parity_reference(pkg, oracle, "uc8")
    caps = [np.concatenate([c, capture(pkg, "uc8", 6300 + r, 1)]) for r, c in enumerate(caps)]
    g, twin = make_group(pkg, "uc8", stage), make_group(pkg, "uc8", stage)
    for c in range(calls):
        order = [(2 * c + k) % K for k in range(K)]
        iq = np.concatenate([buf_of(caps[r], c, 2) for r in order])
        ref = twin.submit(iq, order, as_dict=True)
        if c % 2:
            mine = g.submit(iq, order, as_dict=True)
            assert all(mine[r].tobytes() == ref[r].tobytes() for r in order), f"call {c}"
        else:
            verbatim = c == 2
            got = g.submit_host_wire(iq, order, 0, verbatim=verbatim)
            assert [e[0] for e in got] == order
            for r, data, nmsgs in got:
                assert (data, nmsgs) == host_bytes(host, ref[r], 0, verbatim), (c, r)
    for r in range(K):
        assert g.stats(r) == twin.stats(r)


def test_rescanned_call(pkg, oracle, host):
    """test_gpu_receiver_group_fields.py::test_rescanned_call's construction: a receiver of full-scale noise among quiet
    ones overflows the region slices, the call is scanned again in pieces and every entry is resolved on the host -- its
    bytes come from the host writers on the entry's thread."""
    Kr = 64
    rng = np.random.default_rng(9)
    quiet = [capture(pkg, "uc8", 5500 + r, 2, rate=500, ac_rate=3000) for r in range(Kr)]
    loud = rng.integers(0, 256, size=2 * CHUNK * 2, dtype=np.uint8)
    src = [loud if r == 3 else quiet[r] for r in range(Kr)]
    g = pkg.capi.ReceiverGroup(Kr, fmt=pkg.capi.FMT_UC8, test_arena_permille=40)
    plain = pkg.capi.ReceiverGroup(Kr, fmt=pkg.capi.FMT_UC8, test_arena_permille=40)
    for r in range(1, Kr, 2):
        g.set_receiver_mode_ac(r, 1)
        plain.set_receiver_mode_ac(r, 1)
    n = 0
    assert g.timing()["reruns"] == 0
    for c in range(2):
        iq = np.concatenate([buf_of(src[r], c, 2) for r in range(Kr)])
        ref = plain.submit(iq, range(Kr), as_dict=True)
        got = g.submit_host_wire(iq, range(Kr), 0)
        assert [e[0] for e in got] == list(range(Kr))
        for r, data, nmsgs in got:
            assert (data, nmsgs) == host_bytes(host, ref[r], 0, False), (c, r)
            n += nmsgs
    t = g.timing()
    assert t["reruns"] > 0 and t["resolve_fallback"] >= Kr * t["reruns"]  # every entry of a rescanned call on the host
    assert n > 100
    for r in range(Kr):
        assert g.stats(r) == plain.stats(r)


@pytest.mark.parametrize("stage", STAGES)
def test_empty_entry_and_bad_arguments(pkg, oracle, host, stage):
    capi = pkg.capi
    caps, _, _ = parity_reference(pkg, oracle, "uc8")
    g, twin = make_group(pkg, "uc8", stage), make_group(pkg, "uc8", stage)
    silence = np.full(2 * CHUNK, 127, dtype=np.uint8)
    bufs = lambda c: [silence if r == 1 else buf_of(caps[r], c, 2) for r in range(K)]
    # an entry whose buffer is silence: its sink call comes all the same, with no bytes
    iq = np.concatenate(bufs(0))
    ref = twin.submit(iq, range(K), as_dict=True)
    got = g.submit_host_wire(iq, range(K), 0)
    assert [e[0] for e in got] == list(range(K)) and got[1] == (1, b"", 0) and len(ref[1]) == 0
    for r, data, nmsgs in got:
        assert (data, nmsgs) == host_bytes(host, ref[r], 0, False), r
    assert sum(e[2] for e in got) > 50
    # bad entries and a bad format: -EINVAL with nothing changed
    before = [g.stats(r) for r in range(K)]
    iq = np.concatenate(bufs(1))
    for bad in ([0, 0, 1, 2], [0, 1, 2, 4], [0, 1, 2, 3, 1]):
        with pytest.raises(capi.MsdError, match="-22"):
            g.submit_host_wire(np.concatenate([iq, iq]), bad, 0)
    for fmt, verbatim_flags in ((3, 0), (-1, 0), (0, 2)):
        L = capi._group_lib()
        entries = (capi.GroupEntry * K)(*[capi.GroupEntry(r, 0, 0) for r in range(K)])
        assert L.msd_group_submit_host_wire(g._h, iq.ctypes.data, entries, K, fmt, verbatim_flags, None, None) == -22
        assert L.msd_group_submit_device_wire(g._h, None, entries, K, fmt, verbatim_flags, None, None) == -22
    entries[2].flags = 1
    assert L.msd_group_submit_host_wire(g._h, iq.ctypes.data, entries, K, 0, 0, None, None) == -22
    entries[2].flags = 0
    assert L.msd_group_submit_host_wire(g._h, None, entries, K, 0, 0, None, None) == -22
    assert L.msd_group_submit_device_wire(g._h, C.c_void_p(8), entries, K, 0, 0, None, None) == -22  # not 16-byte aligned
    assert L.msd_group_submit_device_wire(None, None, entries, K, 0, 0, None, None) == -22
    assert [g.stats(r) for r in range(K)] == before
    ref = twin.submit(iq, range(K), as_dict=True)
    got = g.submit_host_wire(iq, range(K), 0, verbatim=True)
    for r, data, nmsgs in got:
        assert (data, nmsgs) == host_bytes(host, ref[r], 0, True), r
    for r in range(K):
        assert g.stats(r) == twin.stats(r)
