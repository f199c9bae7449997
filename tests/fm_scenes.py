"""Constructed sample buffers for the sequential float sums of the 16-bit converters, and their reference -- TEST
INFRASTRUCTURE, numpy only, nothing of the project imported.

The reference follows convert.c:228-242 (SC16) / :345-357 (SC16Q11): x = int16 * (1 / scale) in float, magsq = fl(fl(xI xI) +
fl(xQ xQ)) clamped to 1, m = sqrtf(magsq), and the two sums s = fl(s + v) over the buffer in order
(np.add.accumulate(dtype=float32) is strictly sequential; np.sum is pairwise and would not do).  For the MAGSQ "format"
(what --dcfilter hands to the sums) the input is the float32 squares themselves.

A scene is a function returning (n, 2) int16 I/Q for one buffer of at most BUF samples; its docstring says which property
of the EXACT sums it has.  tests/test_fm_scenes.py asserts those properties from the reference's own prefix sums -- the
exponent and mantissa of the exact running sum at every BLK-sample block boundary -- never from a model of how the kernels
predict."""
import numpy as np

BUF = 131072          # samples per buffer (MODES_MAG_BUF_SAMPLES)
BLK = 1024            # the granularity at which the properties are stated
NBLK = BUF // BLK
FORMATS = ("sc16", "sc16q11", "magsq")
SCALE = {"sc16": np.float32(1.0 / 32768.0), "sc16q11": np.float32(1.0 / 2048.0)}
FULL = (32767, 32767)  # clamped: level and power value exactly 1.0 in SC16 (and in SC16Q11)


# ------------------------------------------------------------------------------------------------------- the reference
def values(fmt, iq):
    """(level values, power values) as float32 arrays: what the converter adds to sum_level / sum_power per sample.
    fmt "magsq": iq is the float32 array of squares."""
    if fmt == "magsq":
        sq = np.ascontiguousarray(iq, dtype=np.float32)
    else:
        x = np.asarray(iq, dtype=np.int16).reshape(-1, 2).astype(np.float32) * SCALE[fmt]
        sq = (x[:, 0] * x[:, 0]).astype(np.float32) + (x[:, 1] * x[:, 1]).astype(np.float32)
        sq = np.minimum(sq.astype(np.float32), np.float32(1.0))
    return np.sqrt(sq, dtype=np.float32), sq


def prefix(v):
    """the running sequential float32 sum behind every element"""
    return np.add.accumulate(np.asarray(v, dtype=np.float32), dtype=np.float32)


def seq_sum(v):
    return prefix(v)[-1] if len(v) else np.float32(0.0)


def sums(fmt, iq):
    """(sum_level, sum_power) of one buffer as float32 scalars"""
    m, sq = values(fmt, iq)
    return np.float32(seq_sum(m)), np.float32(seq_sum(sq))


def sums_bits(fmt, iq):
    return np.array(sums(fmt, iq), dtype=np.float32).view(np.uint32)


def magsq_of(iq):
    """the float32 squares of a scene (its SC16 reading): the MAGSQ input"""
    return values("sc16", iq)[1]


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def block_starts(v):
    """exact running sum at the start of blocks 1, 2, ... and at the end of each of them: (start, end) float32 arrays"""
    p = prefix(v)
    n = len(p)
    k = np.arange(1, (n + BLK - 1) // BLK)
    return p[k * BLK - 1], p[np.minimum((k + 1) * BLK, n) - 1]


def edge_blocks(v):
    """Blocks (from block 1 on) whose exact start sum lies within 2^-10 relative of a power of two (mantissa below 0x2000
    or above 0x7fe000) or whose start and end exponents differ."""
    s, e = block_starts(v)
    sb, eb = bits(s), bits(e)
    mant = sb & 0x7FFFFF
    return int(np.count_nonzero((mant < 0x2000) | (mant > 0x7FE000) | ((sb >> 23) != (eb >> 23))))


def block_totals(fmt, iq, nblk=NBLK):
    """honest float64 totals of every block, [nblk][level, power] (zeros behind the buffer's end), as float32"""
    m, sq = values(fmt, iq)
    out = np.zeros((nblk, 2), dtype=np.float64)
    for j, v in enumerate((m, sq)):
        pad = np.zeros(nblk * BLK, dtype=np.float64)
        pad[: len(v)] = v
        out[:, j] = pad.reshape(nblk, BLK).sum(axis=1)
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ scenes
SCENES = {}


def scene(name, **kw):
    def reg(fn):
        SCENES[name] = (fn, kw)
        return fn
    return reg


def make(name):
    fn, kw = SCENES[name]
    iq = np.ascontiguousarray(fn(**kw), dtype=np.int16)
    assert iq.ndim == 2 and iq.shape[1] == 2 and 0 < len(iq) <= BUF, name
    return iq


def _const(i, q, n=BUF):
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0], out[:, 1] = i, q
    return out


def stagnation(a):
    """64 blocks at full scale (every value exactly 1.0: both sums reach exactly 2^16), then 64 blocks of (a, 0).  a = 32,
    128: every addend is below half a unit of the sum, both sums stay at 65536.0 (real totals 65600 / 65792).  a = 256: the
    level addend is exactly one unit (66048, exact), the power sum stagnates.  a = 384: every level addition is a tie to
    even, the sequential sum is 66560 where the real total is 66304.  The power sum has 75 edge blocks: the second half
    starts every block exactly on 2^16."""
    return np.concatenate([_const(*FULL, 64 * BLK), _const(a, 0, 64 * BLK)])


for _a in (32, 128, 256, 384):
    scene(f"stagnate-a{_a}", a=_a)(stagnation)


@scene("quiet-first-a32", a=32)
@scene("quiet-first-a384", a=384)
def quiet_first(a):
    """The stagnation scene the other way round: 64 blocks of (a, 0) -- a small sum for half a buffer: level 64 / 768, power
    2^-4 / 9 --, then 64 blocks at full scale: the sums run through every binade up to 2^16 inside the second half."""
    return np.concatenate([_const(a, 0, 64 * BLK), _const(*FULL, 64 * BLK)])


@scene("quiet-loud-alternating")
def quiet_loud_alternating():
    """Full-scale blocks and blocks of (1, 0) alternating, a loud one first.  Behind the first loud block a quiet sample
    (level 2^-15, power 2^-30) is below half a unit of either sum, so the sums are exactly 1024 j behind j loud blocks: a
    loud block starts exactly on a power of two at j = 1, 2, 4, ..., 32, ends on one at j + 1 = 2, 4, ..., 64, and the quiet
    block behind such a one starts on it."""
    out = _const(1, 0)
    for b in range(0, NBLK, 2):
        out[b * BLK: (b + 1) * BLK] = FULL
    return out


@scene("zeros")
def all_zero():
    """All zero: both sums are +0 and stay there."""
    return _const(0, 0)


@scene("lsb-i")
def lsb_i():
    """All (1, 0): level 2^-15, power 2^-30 per sample, both sums exact; the power sum ends at 2^-13, below 2^-7 in every
    block."""
    return _const(1, 0)


@scene("lsb-q-negative")
def lsb_q():
    """All (0, -1): the same sums as (1, 0) from the other axis and sign."""
    return _const(0, -1)


def one_sample(pos):
    """Zeros with one full-scale sample at `pos`: both sums are 0 up to it and exactly 1.0 from it on."""
    out = _const(0, 0)
    out[pos] = FULL
    return out


for _p in (0, 1023, 1024, BUF - 1):
    scene(f"one-sample-at-{_p}", pos=_p)(one_sample)


@scene("zero-blocks-between")
def zero_blocks_between():
    """Blocks of (4096, 0) (level 2^-3, power 2^-6) with runs of all-zero blocks between them (one, two, then four zero
    blocks, repeated): a block total of exactly 0 in front of, between and behind non-zero ones."""
    out = _const(4096, 0)
    for b in range(NBLK):
        if b % 10 in (1, 3, 4, 6, 7, 8, 9):
            out[b * BLK: (b + 1) * BLK] = 0
    return out


def pow2_landing(shift):
    """`shift` zero samples, then constant (16384, 0): level 2^-1 and power 2^-2 per sample, every partial sum exact.  The
    level sum is 512 k and the power sum 256 k at sample k BLK + shift: they land exactly on the powers of two up to 2^16 /
    2^15 there -- on the block boundary (shift 0), inside the first lane's sixteen elements (1), at the end, on the boundary
    and at the start of a 64-sample sub-block (63, 64, 65)."""
    out = _const(16384, 0)
    out[:shift] = 0
    return out


for _s in (0, 1, 63, 64, 65):
    scene(f"pow2-landing-shift{_s}", shift=_s)(pow2_landing)


def _behind_loud_prefix(tail):
    """16 full-scale blocks (both sums exactly 2^14, one unit 2^-9 from there to 2^15), then `tail`"""
    out = np.concatenate([_const(*FULL, 16 * BLK), tail])
    assert len(out) == BUF
    return out


@scene("ties-level-parity-alternating")
def ties_level_alternating():
    """Behind 16 full-scale blocks (sum 2^14, unit u = 2^-9): (64, 0), (32, 0) repeated -- level addends u and u / 2.  The
    sum is odd behind every whole unit and the half unit behind it is a tie that rounds up to even: the parity alternates
    with every addition, the sequential sum gains 2 u per pair where the real one gains 1.5 u."""
    tail = _const(64, 0, BUF - 16 * BLK)
    tail[1::2, 0] = 32
    return _behind_loud_prefix(tail)


@scene("ties-level-parity-constant")
def ties_level_constant():
    """Behind 16 full-scale blocks: (96, 0) throughout -- the level addend is 1.5 u, every addition is a tie from an even
    sum and rounds to S + 2: the parity never changes, the sequential sum gains 2 u per sample where the real one gains
    1.5 u."""
    return _behind_loud_prefix(_const(96, 0, BUF - 16 * BLK))


@scene("ties-level-dyadic-mix")
def ties_level_mix():
    """Behind 16 full-scale blocks: amplitudes drawn from {32, 64, 96, 128, 192} = {2^k, 3 2^k} on the I axis (level addends
    u / 2, u, 1.5 u, 2 u, 3 u): ties from even and odd sums in no regular order."""
    rng = np.random.default_rng(55)
    tail = _const(0, 0, BUF - 16 * BLK)
    tail[:, 0] = rng.choice(np.array([32, 64, 96, 128, 192]), size=len(tail))
    return _behind_loud_prefix(tail)


@scene("ties-power-parity-alternating")
def ties_power_alternating():
    """Behind 16 full-scale blocks: (1024, 1024), (1024, 0) repeated -- power addends 2^-9 = u and 2^-10 = u / 2: the power
    sum ties in every second addition, from an odd sum, with the parity alternating."""
    tail = _const(1024, 1024, BUF - 16 * BLK)
    tail[1::2, 1] = 0
    return _behind_loud_prefix(tail)


def one_large(block, offset):
    """Constant (16, 0) -- level 2^-11 and power 2^-22 per sample, 0.5 and 2^-12 per block, every partial sum exact -- with
    one full-scale sample (1.0 / 1.0) at `offset` in `block`: the power sum jumps from below 2^-5 over 1.0, several binades
    inside one lane's sixteen elements, in the middle of a long stretch of equal blocks; the level sum (block / 2 in front
    of the block) leaves its binade there too unless block is 64 or 65."""
    out = _const(16, 0)
    out[block * BLK + offset] = FULL
    return out


ONE_LARGE = sorted({(63, o) for o in (15, 16, 17, 63, 64, 65, 1023)} | {(b, 17) for b in (1, 2, 63, 64, 65, 126, 127)}
                   | {(1, 1023), (127, 1023), (64, 64)})
for _b, _o in ONE_LARGE:
    scene(f"one-large-block{_b}-offset{_o}", block=_b, offset=_o)(one_large)


@scene("saturated-min-min", i=-32768, q=-32768)
@scene("saturated-max-min", i=32767, q=-32768)
@scene("saturated-q11-2047-m2048", i=2047, q=-2048)
def saturated(i, q):
    """Constant (i, q) at the end of the range: SC16 squares above 1 in front of the clamp ((-32768)^2 scaled is exactly 1
    per axis), SC16Q11 with |x| = 16 or just below 1 on both axes.  Every value is 1.0 behind the clamp and the sums are
    exact integers up to 2^17."""
    return _const(i, q)


@scene("saturated-mixed-extremes")
def saturated_mixed():
    """Each axis drawn from {-32768, 32767}: clamped in both formats (SC16: 1 or just below per axis, SC16Q11: |x| = 16),
    every value exactly 1.0."""
    rng = np.random.default_rng(77)
    return rng.choice(np.array([-32768, 32767]), size=(BUF, 2)).astype(np.int16)


def gaussian(fs, seed):
    """Gaussian noise of standard deviation `fs` of the SC16 full scale per axis: the unbiased baseline (every binade
    crossed once, no stagnation)."""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.standard_normal((BUF, 2)) * fs * 32768.0), -32768, 32767).astype(np.int16)


for _k, _fs in enumerate((0.002, 0.05, 0.3)):
    scene(f"noise-{_fs}", fs=_fs, seed=900 + _k)(gaussian)


@scene("uniform-int16")
def uniform_int16():
    """Uniformly random int16 on both axes: about a fifth of the SC16 samples clamp, nearly all SC16Q11 samples do."""
    return np.random.default_rng(31).integers(-32768, 32768, size=(BUF, 2)).astype(np.int16)


NAMES = tuple(SCENES)
