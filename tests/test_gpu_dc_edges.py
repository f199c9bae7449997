"""--dcfilter at the filter states where binary32 behaves differently, against the oracle's in-order converter
(modes_oracle.c convert_dc, convert.c:113-213, 374-423): a fresh context (state +0) whose first samples are zero, one
channel zero, seconds of silence that take the state down to the subnormal floor (190650 * 2^-149, where fl(z * dc_b) = z),
the edges of the input range, and the documented cliff of the passes.  The public path in all three ways (the parallel
passes, the passes in one cooperative launch, the in-order kernel alone), and the pair of launches behind it driven from
explicit start states (white box: msd_launch_dcfilter_parallel, then msd_launch_dcfilter(..., skip_if = work), as
msd_capi.cpp launch_dc_block queues them) -- magnitudes, both means and the end state bit for bit.

Zero and silent blocks are decided exactly by the candidate rule of the walk (the block's start state is one of its
candidates), so there the parallel kernels must finish the batch themselves: dc_filter_status()[0] == 1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import fmt_ids

CHUNK = 131072
MI = 1 << 20
FLOOR = 190650                  # bits of the subnormal floor (tests/test_dc_reference.py pins it)
FLT_MIN = 0x00800000
START_STATES = {"+0": 0x00000000, "-0": 0x80000000, "2^-149": 0x00000001, "floor": FLOOR, "floor+1ulp": FLOOR + 1,
                "FLT_MIN": FLT_MIN, "-3FLT_MIN": 0x81400000, "1e-30": 0x0da24260, "16.0": 0x41800000}
pytestmark = pytest.mark.gpu


def iq_of(fmt, v):
    """(n, 2) float values in units of full scale -> raw little-endian samples (no clipping: callers stay in range)."""
    full = {"sc16": 32768.0, "sc16q11": 2048.0}[fmt]
    return np.rint(np.asarray(v) * full).astype("<i2").reshape(-1).view(np.uint8)


def noise(fmt, n, seed, offset=(0.004, -0.02)):
    rng = np.random.default_rng(seed)
    return iq_of(fmt, np.clip(rng.standard_normal((n, 2)) * 0.05 + np.array(offset), -0.99, 0.99))


def zeros(n):
    return np.zeros(4 * n, dtype=np.uint8)


WAYS = (("default", 0), ("fused", "CFG_DC_FUSED_LAUNCH"), ("sequential", "CFG_DC_SEQUENTIAL"))


class ThreeWays:
    """One oracle context and a Demodulator per way, fed the same calls; every call's magnitudes and means compared."""

    def __init__(self, pkg, oracle, fmt, max_batch, exact=True):
        f, of = fmt_ids(pkg, oracle, fmt)
        self.orc = oracle.Oracle(of, 58, 1, 0, dc_filter=True)
        self.dems = [(name, pkg.Demodulator(fmt=f, nfix_crc=1, max_batch_samples=max_batch, dc_filter=True,
                                            flags=getattr(pkg.capi, flag) if flag else 0)) for name, flag in WAYS]
        self.exact, self.calls = exact, 0

    def convert(self, blk, what=""):
        m = blk.size // 4
        wm, wl, wp = self.orc.convert(blk, m)
        for name, dem in self.dems:
            gm, gl, gp = dem.convert(blk, m)
            status = dem.dc_filter_status()
            where = (what, self.calls, m, name, status)
            if not np.array_equal(gm[:m], wm):
                k = int(np.flatnonzero(gm[:m] != wm)[0])
                raise AssertionError(f"magnitudes differ {where}: first at {k}: {int(gm[k])} != {int(wm[k])}, "
                                     f"{int(np.count_nonzero(gm[:m] != wm))} of {m}")
            assert np.array_equal(np.float64(gl), np.float64(wl), equal_nan=True), (where, gl, wl)
            assert np.array_equal(np.float64(gp), np.float64(wp), equal_nan=True), (where, gp, wp)
            if name == "sequential":
                assert status[0] == 0, where
            elif self.exact:
                assert status[0] == 1, where    # the parallel kernels did it: nothing was handed to the in-order kernel
        self.calls += 1
        return wm

    def close(self):
        for _, dem in self.dems:
            dem.close()
        self.orc.close()


# ---------------------------------------------------------------------------------------------------------------------
# a-f: the public path (msd_convert), call after call
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["sc16", "sc16q11"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, CHUNK, 8 * CHUNK + 777])
def test_fresh_context_all_zero_first_call(pkg, oracle, torch_cuda, fmt, n):
    """(a) state +0, a first call of zeros: F(0) = 0 and F(2^-149) = 2^-149 for the block, the candidate rule decides; then
    three calls of offset noise, to show the context carries a sane state on."""
    t = ThreeWays(pkg, oracle, fmt, 16 * CHUNK)
    t.convert(zeros(n), "zeros")
    assert t.orc.dc_state == (0, 0)
    for k, m in enumerate((CHUNK, 4097, 2 * CHUNK)):
        t.convert(noise(fmt, m, seed=100 + k), "noise")
    t.close()


@pytest.mark.parametrize("fmt", ["sc16", "sc16q11"])
@pytest.mark.parametrize("zero_ch", [0, 1])
@pytest.mark.parametrize("other", ["noise", "offset"])
def test_one_channel_zero(pkg, oracle, torch_cuda, fmt, zero_ch, other):
    """(b) a real-only capture (Q = 0) and the other way round: the zero channel's state stays at +0 throughout."""
    t = ThreeWays(pkg, oracle, fmt, 16 * CHUNK)
    for k, m in enumerate((CHUNK, 4097, 8 * CHUNK + 777, 65)):
        blk = noise(fmt, m, seed=200 + k, offset=(0.0, 0.0) if other == "noise" else (0.03, -0.01)).view("<i2").reshape(-1, 2).copy()
        blk[:, zero_ch] = 0
        t.convert(blk.reshape(-1).view(np.uint8), f"ch{zero_ch} zero")
        assert t.orc.dc_state[zero_ch] == 0
    t.close()


@pytest.mark.parametrize("fmt", ["sc16", "sc16q11"])
@pytest.mark.parametrize("lead", [2048, 4096, 65536])
def test_leading_zeros_inside_the_first_call(pkg, oracle, torch_cuda, fmt, lead):
    """(c) a capture padded with zeros: the first blocks of the first call are silent, the signal starts inside it."""
    t = ThreeWays(pkg, oracle, fmt, 16 * CHUNK)
    n = 2 * CHUNK + 333
    blk = noise(fmt, n, seed=lead)
    blk[:4 * lead] = 0
    t.convert(blk, "leading zeros")
    t.convert(noise(fmt, CHUNK, seed=lead + 1), "noise")
    t.close()


def test_long_silence_after_a_signal(pkg, oracle, torch_cuda):
    """(d) 1 Mi samples of offset noise, 34 Mi zero samples in batches of 2 Mi (14 s of a muted front end), then the signal
    again.  The state decays into the subnormals and ends on the floor (+-190650 * 2^-149) -- asserted through the oracle's
    state before the signal resumes."""
    t = ThreeWays(pkg, oracle, "sc16", 2 * MI)
    t.convert(noise("sc16", MI, seed=5), "signal")
    z = zeros(2 * MI)
    for k in range(17):
        t.convert(z, f"silence {k}")
    assert t.orc.dc_state == (FLOOR, FLOOR | 0x80000000), [hex(b) for b in t.orc.dc_state]
    t.convert(noise("sc16", 2 * MI, seed=6), "signal again")
    t.convert(noise("sc16", CHUNK + 5, seed=7), "signal again")
    t.close()


@pytest.mark.parametrize("case", ["sc16-extremes", "sc16-constant-min", "sc16q11-int16-range", "sc16q11-constant-max"])
def test_edges_of_the_input_range(pkg, oracle, torch_cuda, case):
    """(e) SC16 at -32768 / 32767 in both channels; SC16Q11 over the whole int16 range (|f| up to 16: convert.c:392-395
    divides by 2048 without masking), so the state goes up to about 16."""
    fmt = case.split("-")[0]
    t = ThreeWays(pkg, oracle, fmt, 16 * CHUNK, exact=False)   # (how many passes saturated input takes is not the point here)
    rng = np.random.default_rng(len(case))
    for k, m in enumerate((CHUNK, 4097, 8 * CHUNK + 777)):
        if case == "sc16-extremes":
            v = np.where(rng.random((m, 2)) < 0.5, -32768, 32767)
        elif case == "sc16-constant-min":
            v = np.full((m, 2), -32768)
        elif case == "sc16q11-int16-range":
            v = rng.integers(-32768, 32768, (m, 2))
        else:
            v = np.tile(np.array([32767, -32768]), (m, 1))
        t.convert(v.astype("<i2").reshape(-1).view(np.uint8), case)
    t.close()


def test_the_documented_cliff(pkg, oracle, torch_cuda):
    """(f) SC16 alternating at full scale, one batch of 32 Mi samples: the passes run out (profiles/r06_dc_passes.txt) and
    the in-order kernel takes over where they stopped -- the magnitudes and means are still the oracle's.  One way at a time
    (a 32 Mi batch context each)."""
    n = 32 * MI
    odd = (np.arange(n) & 1) == 1
    v = np.empty((n, 2), dtype="<i2")             # +-1.0 and +-0.5 of full scale, clipped like every SC16 source
    v[:, 0] = np.where(odd, 32767, -32768)
    v[:, 1] = np.where(odd, 16384, -16384)
    blk = v.reshape(-1).view(np.uint8)
    wm, wl, wp = oracle.Oracle(oracle.FMT_SC16, 58, 1, 0, dc_filter=True).convert(blk, n)
    for name, flag in WAYS:
        dem = pkg.Demodulator(fmt=pkg.FMT_SC16, nfix_crc=1, max_batch_samples=n, dc_filter=True,
                              flags=getattr(pkg.capi, flag) if flag else 0)
        gm, gl, gp = dem.convert(blk, n)
        assert np.array_equal(gm[:n], wm), (name, dem.dc_filter_status(), int(np.count_nonzero(gm[:n] != wm)))
        assert gl == wl and gp == wp, (name, gl, wl, gp, wp)
        dem.close()


# ---------------------------------------------------------------------------------------------------------------------
# white box: the pair of launches from explicit start states
# ---------------------------------------------------------------------------------------------------------------------

def dcp_lib(pkg):
    L = C.CDLL(pkg.capi.LIB_PATH)
    L.msd_dcp_work_bytes.restype = C.c_size_t
    L.msd_dcp_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
    L.msd_launch_dcfilter_parallel.restype = C.c_int
    L.msd_launch_dcfilter_parallel.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.msd_launch_dcfilter.restype = C.c_int
    L.msd_launch_dcfilter.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    return L


DC_B = np.float32(np.exp(-2 * np.pi / 2.4e6))
DC_A = np.float32(1.0 - float(DC_B))
WB_CONTENTS = ("zero", "one_zero", "lsb", "offset", "full")
FIXED_POINTS = ("+0", "-0", "2^-149", "floor", "floor+1ulp")   # zero input: every block starts on one of its candidates


def wb_content(kind, n, seed):
    """(format, raw samples): SC16 but for full scale, which is SC16Q11 over the int16 range (|f| up to 16)."""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return "sc16", zeros(n)
    if kind == "one_zero":
        v = np.zeros((n, 2), dtype="<i2")
        v[:, 0] = np.rint(rng.standard_normal(n) * 1600 + 130).astype("<i2")
        return "sc16", v.reshape(-1).view(np.uint8)
    if kind == "lsb":
        v = np.where((np.arange(n) & 1)[:, None] == 1, 1, -1) * np.array([1, -1])
        return "sc16", v.astype("<i2").reshape(-1).view(np.uint8)
    if kind == "offset":
        return "sc16", noise("sc16", n, seed)
    if kind == "full":
        return "sc16q11", rng.integers(-32768, 32768, (n, 2)).astype("<i2").reshape(-1).view(np.uint8)
    raise ValueError(kind)


@pytest.mark.parametrize("block_len", [64, 192, 1024, 2048, 4096, 32768, 65536])
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("max_passes", [1, 2, 24])
def test_parallel_dc_pair_from_explicit_states(pkg, oracle, torch_cuda, block_len, fused, max_passes):
    """msd_launch_dcfilter_parallel + msd_launch_dcfilter(skip_if = work) from every start state of the list, on zero, one
    channel zero, +-1 LSB, offset and full-scale content: the magnitudes and the END STATE bits are the oracle's from the same
    start.  Block lengths that meet the documented contract (a multiple of 64) but not the 256-sample group included.  Zero
    content from a fixed point of the map is exact in the first pass, so the passes must have finished it."""
    L = dcp_lib(pkg)
    n = 4 * block_len + 77
    work = torch_cuda.zeros(L.msd_dcp_work_bytes(n, block_len), dtype=torch_cuda.uint8, device="cuda")
    mag = torch_cuda.zeros(n, dtype=torch_cuda.int16, device="cuda")
    sq = torch_cuda.zeros(n, dtype=torch_cuda.float32, device="cuda")
    for ki, kind in enumerate(WB_CONTENTS):
        fmt, iq = wb_content(kind, n, seed=block_len + ki)
        f, of = fmt_ids(pkg, oracle, fmt)
        d_iq = torch_cuda.from_numpy(iq.copy()).cuda()
        for name, bits in START_STATES.items():
            start = np.array([bits, bits], dtype=np.uint32)
            orc = oracle.Oracle(of, 58, 1, 0, dc_filter=True)
            orc.dc_state = tuple(int(b) for b in start)
            wm = orc.convert(iq, n)[0]
            want_state = orc.dc_state
            orc.close()
            state = torch_cuda.from_numpy(start.view(np.float32).copy()).cuda()
            where = (kind, name, block_len, fused, max_passes)
            assert L.msd_launch_dcfilter_parallel(f, d_iq.data_ptr(), n, float(DC_A), float(DC_B), state.data_ptr(), mag.data_ptr(),
                                                  sq.data_ptr(), work.data_ptr(), block_len, max_passes, fused, None) == 0, where
            assert L.msd_launch_dcfilter(f, d_iq.data_ptr(), n, float(DC_A), float(DC_B), state.data_ptr(), mag.data_ptr(),
                                         sq.data_ptr(), work.data_ptr(), None) == 0, where
            torch_cuda.cuda.synchronize()
            got_state = tuple(int(b) for b in state.cpu().numpy().view(np.uint32))
            gm = mag.cpu().numpy().view(np.uint16)
            done = int(work[:4].cpu().numpy().view(np.uint32)[0])
            if not np.array_equal(gm, wm):
                k = int(np.flatnonzero(gm != wm)[0])
                raise AssertionError(f"magnitudes differ {where} (done {done}): first at {k}: {int(gm[k])} != {int(wm[k])}, "
                                     f"end state {[hex(b) for b in got_state]} want {[hex(b) for b in want_state]}")
            assert got_state == want_state, (where, done, [hex(b) for b in got_state], [hex(b) for b in want_state])
            if kind == "zero" and name in FIXED_POINTS:
                assert done == 1, where


def test_a_block_length_off_the_contract_is_refused(pkg, torch_cuda):
    """The argument check of msd_launch_dcfilter_parallel: a block shorter than 64 samples or not a multiple of 64 is -EINVAL
    (the fine states are one per 64 samples), and nothing is launched."""
    L = dcp_lib(pkg)
    n = 4096
    d_iq = torch_cuda.zeros(4 * n, dtype=torch_cuda.uint8, device="cuda")
    work = torch_cuda.zeros(L.msd_dcp_work_bytes(n, 64), dtype=torch_cuda.uint8, device="cuda")
    state = torch_cuda.zeros(2, dtype=torch_cuda.float32, device="cuda")
    mag = torch_cuda.zeros(n, dtype=torch_cuda.int16, device="cuda")
    sq = torch_cuda.zeros(n, dtype=torch_cuda.float32, device="cuda")
    for bad in (0, 1, 32, 63, 65, 96, 1000):
        assert L.msd_launch_dcfilter_parallel(pkg.FMT_SC16, d_iq.data_ptr(), n, float(DC_A), float(DC_B), state.data_ptr(), mag.data_ptr(),
                                              sq.data_ptr(), work.data_ptr(), bad, 2, 0, None) == -22, bad


# ---------------------------------------------------------------------------------------------------------------------
# the stream interface and the replay tool
# ---------------------------------------------------------------------------------------------------------------------

def silent_start_capture(pkg):
    n = 10 * CHUNK + 4321
    iq = pkg.siggen.generate(pkg.siggen.make_cfg(seed=4242, fmt=pkg.siggen.SC16, msgs_per_sec=5000, n_aircraft=40), n)
    iq[:4 * 8192] = 0           # the first 8192 samples zero in both channels: the first blocks of a fresh context are silent
    return iq, n


def test_silent_start_in_the_stream_interface(pkg, oracle, torch_cuda):
    """msd_launch_device of a --dcfilter SC16 context, three batches pipelined, a capture whose first 8192 samples are zero:
    the message list is the oracle's, every batch exact."""
    iq, n = silent_start_capture(pkg)
    d_iq = torch_cuda.from_numpy(iq).to("cuda:0")
    dem = pkg.Demodulator(fmt=pkg.FMT_SC16, nfix_crc=1, max_batch_samples=4 * CHUNK, message_capacity=1 << 16, dc_filter=True)
    off = 0
    for m, last in ((4 * CHUNK, False), (4 * CHUNK, False), (n - 8 * CHUNK, True)):
        dem.launch_device(d_iq.data_ptr() + 4 * off, m, last=last)
        assert dem.dc_filter_status()[0] == 1
        off += m
    got = np.concatenate([dem.collect() for _ in range(3)])
    want, _ = oracle.Oracle(oracle.FMT_SC16, 58, 1, 0, dc_filter=True).replay(iq, cap=1 << 16)
    assert len(want) >= 100
    assert len(got) == len(want) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("path", ["fused", "magbuf"])
def test_silent_start_through_the_replay_tool(pkg, oracle, torch_cuda, tmp_path, path):
    """msd_replay --iformat sc16 --dcfilter --mlat --raw on the same capture, both paths: the oracle's messages, line by line."""
    iq, _ = silent_start_capture(pkg)
    f = tmp_path / "capture.sc16"
    iq.tofile(f)
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    out = subprocess.run([exe, "--ifile", str(f), "--iformat", "sc16", "--dcfilter", "--mlat", "--raw", "--path", path],
                         capture_output=True, text=True, check=True, timeout=300)
    want, _ = oracle.Oracle(oracle.FMT_SC16, 58, 1, 0, dc_filter=True).replay(iq, cap=1 << 16)
    lines = out.stdout.split()
    assert len(lines) == len(want) >= 100
    for line, m in zip(lines, want):
        assert line == "@%012X%s;" % (int(m["timestampMsg"]), bytes(m["msg"][: m["msgbits"] // 8]).hex())
