"""--dcfilter without a GPU: the oracle's in-order DC block (modes_oracle.c convert_dc, convert.c:113-213, 374-423) pinned
by exact arithmetic at the filter states where binary32 behaves differently -- zero of either sign, subnormal, the floor
where silence leaves the state, the smallest normal, beyond full scale -- and the block-length / workspace arithmetic of
the parallel DC block (msd_dc_kernels.hip msd_dcp_block_len, msd_dcp_work_bytes).

The exact reference is built from fractions.Fraction and an explicit round-to-nearest-even to binary32, subnormals
included, and carries the sign of a zero by hand.  Agreement with it also shows that this process does not flush
subnormals (no FTZ / DAZ in the MXCSR): every GPU comparison against the oracle rests on that."""
import ctypes as C
import math
import struct
from fractions import Fraction

import pytest

# ---------------------------------------------------------------------------------------------------------------------
# binary32 by exact arithmetic: a value is (Fraction, sign bit); the sign bit only matters for a zero
# ---------------------------------------------------------------------------------------------------------------------
EMIN, MANT = -126, 23           # the smallest normal exponent, the explicit mantissa bits
FLT_MAX = Fraction((1 << 24) - 1) * Fraction(2) ** (127 - 23)


def _floor_log2(a):
    """e with 2^e <= a < 2^(e + 1), a > 0."""
    n, d = a.numerator, a.denominator
    e = n.bit_length() - d.bit_length()
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1
    return e


def rnd(x, neg_if_zero=False):
    """x (exact) rounded to the nearest binary32, ties to even; subnormals are kept, nothing is flushed."""
    if x == 0:
        return (Fraction(0), neg_if_zero)
    neg = x < 0
    a = -x if neg else x
    q = max(_floor_log2(a), EMIN) - MANT            # the quantum: 2^q
    s = a / Fraction(2) ** q
    m, r = divmod(s.numerator, s.denominator)
    if 2 * r > s.denominator or (2 * r == s.denominator and m & 1):
        m += 1
    v = Fraction(m) * Fraction(2) ** q
    assert v <= FLT_MAX, "overflow is not expected in the DC block"
    return (-v if neg else v, neg)


def add(a, b):
    x = a[0] + b[0]
    if x == 0:  # an exact zero sum is +0 under round-to-nearest, but for (-0) + (-0)
        return (Fraction(0), a[0] == 0 and b[0] == 0 and a[1] and b[1])
    return rnd(x)


def sub(a, b):
    return add(a, (-b[0], not b[1]))


def mul(a, b):
    return rnd(a[0] * b[0], a[1] != b[1])


def div(a, b):
    return rnd(a[0] / b[0], a[1] != b[1])


def sqrt(a):
    """Correctly rounded square root of a >= 0 (sqrt(-0) = -0)."""
    if a[0] == 0:
        return a
    q = max(_floor_log2(a[0]) // 2, EMIN) - MANT
    t = a[0] / Fraction(4) ** q                     # sqrt(a) / 2^q = sqrt(t)
    m = math.isqrt(t.numerator // t.denominator)    # floor(sqrt(t))
    h = (Fraction(2 * m + 1, 2)) ** 2
    if t > h or (t == h and m & 1):
        m += 1
    return (Fraction(m) * Fraction(2) ** q, False)


def from_bits(u):
    """binary32 bits -> exact value (finite only)."""
    neg, e, f = u >> 31, (u >> 23) & 0xff, u & 0x7fffff
    assert e != 0xff
    v = Fraction(f) * Fraction(2) ** (EMIN - MANT) if e == 0 else Fraction(f | 1 << 23) * Fraction(2) ** (e - 127 - MANT)
    return (-v if neg else v, bool(neg))


def to_bits(a):
    v, neg = a
    if v == 0:
        return 0x80000000 if neg else 0
    u = 0x80000000 if v < 0 else 0
    v = abs(v)
    if v < Fraction(2) ** EMIN:
        return u | int(v / Fraction(2) ** (EMIN - MANT))
    e = _floor_log2(v)
    return u | (e + 127) << 23 | int(v / Fraction(2) ** (e - MANT)) - (1 << 23)


def lit(x):
    """A C float literal or int converted to float."""
    return rnd(Fraction(x))


# dc_b = exp(-2 pi / 2.4e6) in double, stored in a float; dc_a = 1.0 - dc_b in double, stored in a float
# (orc_set_dc_filter, convert.c:479-482)
DC_B = rnd(Fraction(math.exp(-2.0 * math.pi * 1.0 / 2400000.0)))
DC_A = rnd(1 - DC_B[0])
ULP0 = Fraction(2) ** (EMIN - MANT)             # 2^-149
FLOOR = 190650                                   # z = FLOOR * 2^-149: fl(z * dc_b) = z, and nothing above it stays put


def sample_value(fmt, raw):
    """convert.c:133-134 (UC8: (I - 127.5f) / 127.5f, a real division) and :183-184 / :392-395 (I / 32768.0f, I / 2048.0f)."""
    if fmt == "uc8":
        return div(sub(lit(raw), lit(Fraction(255, 2))), lit(Fraction(255, 2)))
    return div(lit(raw), lit(32768 if fmt == "sc16" else 2048))


def exact_convert(fmt, iq, z):
    """convert_*_generic step by step: z <- fl(fl(f * a) + fl(z * b)) per channel, the magnitude, the u16, the float sums
    and their float means.  iq: list of (I, Q) raw values; z: [zi, zq] exact values.  Returns (mag, ml, mp, z)."""
    one, scale, half = lit(1), lit(65535), lit(Fraction(1, 2))
    cache = {}
    zi, zq = z
    sum_level = sum_power = lit(0)
    mags = []
    for I, Q in iq:
        for raw in (I, Q):
            if raw not in cache:
                cache[raw] = sample_value(fmt, raw)
        fi, fq = cache[I], cache[Q]
        zi = add(mul(fi, DC_A), mul(zi, DC_B))
        zq = add(mul(fq, DC_A), mul(zq, DC_B))
        di, dq = sub(fi, zi), sub(fq, zq)
        magsq = add(mul(di, di), mul(dq, dq))
        if magsq[0] > 1:
            magsq = one
        m = sqrt(magsq)
        sum_power = add(sum_power, magsq)
        sum_level = add(sum_level, m)
        mags.append(int(add(mul(m, scale), half)[0]))       # (uint16_t)(m * 65535.0f + 0.5f): truncation, m <= 1
    n = lit(len(iq))
    return mags, div(sum_level, n)[0], div(sum_power, n)[0], [zi, zq]


# ---------------------------------------------------------------------------------------------------------------------

def test_the_exact_reference_itself():
    """The pieces the comparison rests on: the filter constants are the floats the oracle and the kernels use, the floor is
    where the text says (a fixed point of z -> fl(z * b), its successor is not), a few roundings of known result."""
    b_bits = struct.unpack("<I", struct.pack("<f", math.exp(-2.0 * math.pi / 2400000.0)))[0]
    assert to_bits(DC_B) == b_bits and DC_A[0] == 1 - DC_B[0]
    assert 1 - DC_B[0] == 44 * Fraction(2) ** -24
    z = (FLOOR * ULP0, False)
    assert mul(z, DC_B) == z
    assert mul(((FLOOR + 1) * ULP0, False), DC_B)[0] == FLOOR * ULP0
    assert mul((ULP0, False), DC_B)[0] == ULP0                  # F(1 ulp) = 1 ulp: the flat-looking bottom of the line
    assert rnd(ULP0 / 2)[0] == 0 and rnd(ULP0 * 3 / 2)[0] == 2 * ULP0   # ties to even at the very bottom
    assert add((Fraction(0), True), (Fraction(0), True)) == (0, True)
    assert add((Fraction(0), False), (Fraction(0), True)) == (0, False)
    for u in (0, 1, FLOOR, 0x007fffff, 0x00800000, 0x80000003, 0x3f800000, 0x41800000, 0x7f7fffff, 0xc0490fdb):
        assert to_bits(from_bits(u)) == u
    for x in (2.0, 0.5, 1e-30, 0.3):
        assert to_bits(sqrt(lit(Fraction(x)))) == struct.unpack("<I", struct.pack("<f", math.sqrt(struct.unpack("<f", struct.pack("<f", x))[0])))[0]


FLT_MIN_BITS = 0x00800000
START_STATES = {
    "+0": 0x00000000,
    "-0": 0x80000000,
    "2^-149": 0x00000001,
    "floor": FLOOR,
    "floor+1ulp": FLOOR + 1,
    "FLT_MIN": FLT_MIN_BITS,
    "-3FLT_MIN": to_bits(mul(lit(-3), from_bits(FLT_MIN_BITS))),
    "1e-30": to_bits(lit(Fraction(1e-30))),
    "16.0": 0x41800000,
}
STEPS = 1500


def raw_input(fmt, kind, n):
    """(I, Q) raw values: all-zero words (for UC8 that is full scale, -1.0: a UC8 sample is never zero), one LSB either side
    of zero alternating (UC8: 127 / 128), or one channel zero with a slow ramp in the other."""
    zero = 0
    if kind == "zero":
        return [(zero, zero)] * n
    if kind == "lsb":
        lo, hi = (127, 128) if fmt == "uc8" else (-1, 1)
        return [(hi, lo) if k & 1 else (lo, hi) for k in range(n)]
    if kind == "one_zero":
        span = 256 if fmt == "uc8" else 4096
        return [(((37 * k) % span) - (0 if fmt == "uc8" else span // 2), zero) for k in range(n)]
    raise ValueError(kind)


def pack(fmt, iq):
    if fmt == "uc8":
        return bytes(v for pair in iq for v in pair)
    return struct.pack("<%dh" % (2 * len(iq)), *(v for pair in iq for v in pair))


@pytest.mark.parametrize("fmt", ["uc8", "sc16", "sc16q11"])
@pytest.mark.parametrize("kind", ["zero", "lsb", "one_zero"])
def test_oracle_dc_block_equals_exact_arithmetic(oracle, fmt, kind):
    """From each start state (both channels), STEPS samples in two calls: the oracle's u16 magnitudes, both means and the end
    state (read through orc_get_dc_state, bit for bit) are what exact arithmetic rounded to binary32 gives."""
    import numpy as np
    of = {"uc8": oracle.FMT_UC8, "sc16": oracle.FMT_SC16, "sc16q11": oracle.FMT_SC16Q11}[fmt]
    iq = raw_input(fmt, kind, STEPS)
    cut = 1000
    for name, bits in START_STATES.items():
        orc = oracle.Oracle(of, 58, 1, 0, dc_filter=True)
        assert orc.dc_state == (0, 0)                              # orc_set_dc_filter resets the state
        orc.dc_state = (bits, bits ^ 0x80000000 if name == "-3FLT_MIN" else bits)
        z = [from_bits(b) for b in orc.dc_state]
        assert [to_bits(v) for v in z] == [bits, bits ^ 0x80000000 if name == "-3FLT_MIN" else bits]
        for part in (iq[:cut], iq[cut:]):
            gm, gl, gp = orc.convert(np.frombuffer(pack(fmt, part), dtype=np.uint8), len(part))
            wm, wl, wp, z = exact_convert(fmt, part, z)
            assert gm.tolist() == wm, (fmt, kind, name, next(k for k in range(len(wm)) if gm[k] != wm[k]))
            assert Fraction(gl) == wl and Fraction(gp) == wp, (fmt, kind, name)
            assert orc.dc_state == tuple(to_bits(v) for v in z), (fmt, kind, name, [hex(b) for b in orc.dc_state],
                                                                  [hex(to_bits(v)) for v in z])
        orc.close()


def test_dc_state_round_trips_every_bit_pattern(oracle):
    """Oracle.dc_state is the two float32 bit patterns: -0 and NaN payloads survive the setter and the getter."""
    orc = oracle.Oracle(oracle.FMT_SC16, 58, 1, 0, dc_filter=True)
    for bits in ((0x80000000, 0), (0x7fc00001, 0xffc00000), (1, 0x80000001), (0x7f7fffff, 0xff800000)):
        orc.dc_state = bits
        assert orc.dc_state == bits


def test_silence_reaches_the_floor(oracle):
    """A premise of the GPU tests of long silence: zero input takes the state down to +-FLOOR * 2^-149 (not to zero), and
    there it stays."""
    import numpy as np
    orc = oracle.Oracle(oracle.FMT_SC16, 58, 1, 0, dc_filter=True)
    orc.dc_state = (to_bits(lit(Fraction(1, 4096))), to_bits(lit(Fraction(-1, 64))))
    zeros = np.zeros(4 * (1 << 22), dtype=np.uint8)
    for _ in range(8):
        orc.convert(zeros, 1 << 22)
    assert orc.dc_state == (FLOOR, FLOOR | 0x80000000)
    orc.convert(zeros, 1 << 22)
    assert orc.dc_state == (FLOOR, FLOOR | 0x80000000)


# ---------------------------------------------------------------------------------------------------------------------
# block length and workspace of the parallel DC block (the library loads without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
MI = 1 << 20
BLOCK_LEN_N = (1, 63, 64, 65535, 65536, 65537, 2 * MI - 1, 2 * MI, 2 * MI + 1, 2 * MI + 2048, 32 * MI - 1, 32 * MI,
               32 * MI + 1, 32 * MI + 32767, 32 * MI + 32768, 64 * MI - 1, 64 * MI, 64 * MI + 1, 64 * MI + 32767,
               64 * MI + 32768, 128 * MI - 1, 128 * MI, 128 * MI + 1, 256 * MI)


def dcp_e_offset(nb):
    """msd_dc_kernels.hip dcp_e_offset: 256 bytes of control words, then S, cen, ever (2 x nb words each), 256-aligned."""
    return 256 + ((nb * 2 * 4 * 3 + 255) & ~255)


def dcp_bytes_used(n, L):
    """What dcp_launch addresses for a batch of n samples in blocks of L: the tables E (2 x nb x 64 float4) behind
    dcp_e_offset(nb), then the states at every 64th sample (2 x ceil(n / 64) words)."""
    nb = -(-n // L)
    nfine = -(-n // 64)
    return dcp_e_offset(nb) + nb * 2 * 64 * 16 + nfine * 2 * 4


@pytest.fixture(scope="module")
def dcp_lib(pkg):
    L = C.CDLL(pkg.capi.LIB_PATH)
    L.msd_dcp_work_bytes.restype = C.c_size_t
    L.msd_dcp_work_bytes.argtypes = [C.c_uint64, C.c_uint32]
    L.msd_dcp_block_len.restype = C.c_uint32
    L.msd_dcp_block_len.argtypes = [C.c_uint64]
    return L


@pytest.mark.parametrize("n", BLOCK_LEN_N)
def test_dc_block_length_and_workspace(dcp_lib, n):
    """At every switch of msd_dcp_block_len's regime and next to it: the block length is a power of two in [1024, 65536]
    (a multiple of the 64-sample fine block), the ceil(n / L) blocks -- a one-sample last block counted -- fit the workspace
    msd_create sizes for any batch limit >= n (msd_dcp_work_bytes(max, 0)), and the sized-for-L workspace as well."""
    L = dcp_lib.msd_dcp_block_len(n)
    assert L & (L - 1) == 0 and 1024 <= L <= 65536 and L % 64 == 0, (n, L)
    nb = -(-n // L)                                        # a last block of one sample (2 Mi + 1, 128 Mi + 1) is a block
    need = dcp_bytes_used(n, L)
    for limit in (n, n + 1, n + L, 2 * n, max(n, 256 * MI)):
        assert need <= dcp_lib.msd_dcp_work_bytes(limit, 0), (n, L, limit)
    assert need <= dcp_lib.msd_dcp_work_bytes(n, L)
    # the block count the comment of msd_dcp_work_bytes promises: at most 1025 below 32 Mi samples, blocks of 32768 or more beyond
    if n < 32 * MI:
        assert nb <= 1025, (n, L, nb)
    else:
        assert L >= 32768 and nb <= n // 32768 + 2, (n, L, nb)


def test_dc_block_length_is_monotone(dcp_lib):
    """A longer batch never gets a shorter block (a batch limit's workspace then holds every shorter batch)."""
    prev = 0
    for n in sorted(set(BLOCK_LEN_N) | {k * 131072 + d for k in range(1, 1025, 7) for d in (-1, 0, 1)}):
        L = dcp_lib.msd_dcp_block_len(n)
        assert L >= prev, n
        prev = L
