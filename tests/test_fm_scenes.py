"""The constructed buffers of tests/fm_scenes.py really have the properties they are built for -- asserted from the
reference's own sequential prefix sums --, and three independent statements of the sums agree on every one of them before
the GPU is asked (tests/test_gpu_fm_scenes.py): the numpy reference of fm_scenes.py, the oracle's converter
(modes_oracle.c convert_s16) and the float converters of the second reading (indep_demod.convert + buffer_means)."""
import numpy as np
import pytest

import fm_scenes as S
import indep_demod

F32 = np.float32


def exponent(x):
    return int(S.bits(F32(x)) >> 23) - 127


def mantissa(x):
    return int(S.bits(F32(x)) & 0x7FFFFF)


def rounded_real_sum(v):
    return F32(np.sum(np.asarray(v, dtype=np.float64)))


@pytest.fixture(scope="module")
def scenes():
    return {name: S.make(name) for name in S.NAMES}


def test_every_scene_is_documented_and_distinct(scenes):
    assert len(S.NAMES) >= 40
    for name in S.NAMES:
        assert (S.SCENES[name][0].__doc__ or "").strip(), name
    assert len({scenes[n].tobytes() for n in S.NAMES}) == len(S.NAMES)


@pytest.mark.parametrize("a,level,power", [(32, 65536.0, 65536.0), (128, 65536.0, 65536.0), (256, 66048.0, 65536.0),
                                           (384, 66560.0, 65536.0)])
def test_stagnation_behind_full_scale(scenes, a, level, power):
    iq = scenes[f"stagnate-a{a}"]
    m, sq = S.values("sc16", iq)
    assert (m[: 64 * S.BLK] == 1.0).all() and (sq[: 64 * S.BLK] == 1.0).all()          # clamped to exactly 1
    assert S.prefix(m)[64 * S.BLK - 1] == 65536.0 and S.prefix(sq)[64 * S.BLK - 1] == 65536.0
    sl, sp = S.sums("sc16", iq)
    assert (sl, sp) == (F32(level), F32(power))
    real = 65536.0 + 65536 * a / 32768.0
    assert float(np.sum(m, dtype=np.float64)) == real
    if a != 256:
        assert float(sl) != real                                                            # stagnation / ties to even
    # more edge blocks than the kernels keep sub-block functions for (FM_SLOTS = 24 per sum)
    assert S.edge_blocks(sq) == 75
    assert max(S.edge_blocks(m), S.edge_blocks(sq)) >= 25


@pytest.mark.parametrize("name", ["quiet-first-a32", "quiet-first-a384"])
def test_quiet_part_first(scenes, name):
    m, sq = S.values("sc16", scenes[name])
    half = 64 * S.BLK - 1
    assert S.prefix(sq)[half] <= 9.0 and S.prefix(m)[half] <= 768.0
    for v in (m, sq):
        starts, ends = S.block_starts(v)
        crossed = {exponent(x) for x in ends[63:]} - {exponent(starts[62])}
        assert len(crossed) >= 6                                                            # many binades in the loud half
    assert S.sums("sc16", scenes[name])[1] >= 65536.0


def test_quiet_and_loud_blocks_alternating(scenes):
    m, sq = S.values("sc16", scenes["quiet-loud-alternating"])
    for v in (m, sq):
        p = S.prefix(v)
        k = np.arange(1, S.NBLK + 1)
        assert np.array_equal(p[k * S.BLK - 1], (1024.0 * ((k + 1) // 2)).astype(F32))      # exactly 1024 j
        assert S.edge_blocks(v) >= 12
        assert S.seq_sum(v) == 65536.0
    assert rounded_real_sum(m) == 65538.0                                                  # what the quiet blocks really hold


def test_nearly_silent_buffers(scenes):
    assert S.sums_bits("sc16", scenes["zeros"]).tolist() == [0, 0]
    for name in ("lsb-i", "lsb-q-negative"):
        m, sq = S.values("sc16", scenes[name])
        sl, sp = S.sums("sc16", scenes[name])
        assert sl == F32(4.0) and sp == F32(2.0 ** -13)
        assert exponent(S.prefix(sq).max()) < -7                                           # the power sum never reaches 2^-7
    for pos in (0, 1023, 1024, S.BUF - 1):
        m, sq = S.values("sc16", scenes[f"one-sample-at-{pos}"])
        for v in (m, sq):
            p = S.prefix(v)
            assert (p[:pos] == 0).all() and (p[pos:] == 1.0).all()
    tot = S.block_totals("sc16", scenes["zero-blocks-between"])
    zero = (tot[:, 0] == 0) & (tot[:, 1] == 0)
    assert 30 < zero.sum() < S.NBLK - 30 and not zero[0] and zero[1] and zero[-1] and not zero[2]


@pytest.mark.parametrize("shift", [0, 1, 63, 64, 65])
def test_sums_land_exactly_on_powers_of_two(scenes, shift):
    m, sq = S.values("sc16", scenes[f"pow2-landing-shift{shift}"])
    for v, per_block in ((m, 512.0), (sq, 256.0)):
        p = S.prefix(v)
        hits = []
        for k in range(1, S.NBLK):
            at = p[k * S.BLK + shift - 1]                                                  # behind sample k BLK + shift - 1
            assert at == F32(per_block * k)
            if mantissa(at) == 0:
                hits.append(k)
        assert hits == [1, 2, 4, 8, 16, 32, 64]
        assert S.seq_sum(v) == rounded_real_sum(v)                                         # exact throughout


@pytest.mark.parametrize("name,which", [("ties-level-parity-alternating", 0), ("ties-level-parity-constant", 0),
                                        ("ties-level-dyadic-mix", 0), ("ties-power-parity-alternating", 1),
                                        ("stagnate-a384", 0)])
def test_ties_in_every_addition(scenes, name, which):
    """The sequential float32 sum differs from the real (float64, exact here) sum rounded once: round-to-even at work."""
    v = S.values("sc16", scenes[name])[which]
    p = S.prefix(v)
    assert S.bits(p[-1]) != S.bits(rounded_real_sum(v))
    start = 64 * S.BLK if name.startswith("stagnate") else 16 * S.BLK
    unit = F32(2.0) ** (exponent(p[start - 1]) - 23)
    assert exponent(p[-1]) == exponent(p[start - 1])                                       # one binade, one unit throughout
    twice = v[start:].astype(np.float64) / float(unit) * 2
    assert (twice == np.rint(twice)).all()
    ties = np.rint(twice).astype(np.int64) & 1                                             # odd multiples of half a unit
    assert ties.mean() >= 0.3
    parity = ((S.bits(p[start - 1:-1]) & 1) != 0)[ties == 1]                               # of the sum in front of each tie
    if "alternating" in name:
        assert parity.all()                                                                # whole units in between flip it
    elif "constant" in name or name.startswith("stagnate"):
        assert not parity.any()
    else:
        assert 0.2 < parity.mean() < 0.8


@pytest.mark.parametrize("block,offset", S.ONE_LARGE)
def test_one_large_sample_leaves_the_binade_inside_a_lane(scenes, block, offset):
    m, sq = S.values("sc16", scenes[f"one-large-block{block}-offset{offset}"])
    pos = block * S.BLK + offset
    pp = S.prefix(sq)
    assert exponent(pp[pos - 1]) <= -6 and exponent(pp[pos]) == 0                        # the power sum: over several binades
    pl = S.prefix(m)
    assert pl[pos - 1] == F32(pos / 2048.0)
    assert (exponent(pl[pos - 1]) != exponent(pl[pos])) == (block not in (64, 65))
    for v in (m, sq):
        assert S.seq_sum(v) == rounded_real_sum(v)                                         # dyadic and small: still exact


@pytest.mark.parametrize("name", ["saturated-min-min", "saturated-max-min", "saturated-q11-2047-m2048",
                                  "saturated-mixed-extremes"])
def test_saturation(scenes, name):
    iq = scenes[name]
    for fmt in ("sc16", "sc16q11"):
        if name == "saturated-q11-2047-m2048" and fmt == "sc16":
            continue
        m, sq = S.values(fmt, iq)
        assert (sq == 1.0).all() and (m == 1.0).all()
        assert S.sums(fmt, iq) == (F32(S.BUF), F32(S.BUF))
    x = iq.astype(np.float64) / 2048.0
    assert np.abs(x).max() >= 0.999 and ((x * x).sum(axis=1) > 1.0).all()                  # above 1 in front of the clamp
    if name != "saturated-q11-2047-m2048":
        assert np.abs(x).max() == 16.0


def test_noise_is_the_unbiased_baseline(scenes):
    for name in ("noise-0.002", "noise-0.05", "noise-0.3", "uniform-int16"):
        m, sq = S.values("sc16", scenes[name])
        for v in (m, sq):
            assert S.edge_blocks(v) <= 24 and S.seq_sum(v) > 0
    assert exponent(S.sums("sc16", scenes["noise-0.002"])[1]) < 1 < exponent(S.sums("sc16", scenes["noise-0.3"])[1])


def test_the_three_properties_the_gpu_test_relies_on(scenes):
    """At least one scene with more than 24 edge blocks in a sum, one whose sequential sum is not the rounded real sum, one
    whose power sum ends below 2^-7."""
    many = [n for n in S.NAMES if max(S.edge_blocks(v) for v in S.values("sc16", scenes[n])) >= 25]
    uneven = [n for n in S.NAMES if any(S.bits(S.seq_sum(v)) != S.bits(rounded_real_sum(v)) for v in S.values("sc16", scenes[n]))]
    tiny = [n for n in S.NAMES if 0 < S.sums("sc16", scenes[n])[1] < 2.0 ** -7]
    assert len(many) >= 4 and len(uneven) >= 8 and len(tiny) >= 2, (many, uneven, tiny)


@pytest.mark.parametrize("fmt", ["sc16", "sc16q11"])
@pytest.mark.parametrize("name", S.NAMES)
def test_reference_oracle_and_second_reading_agree(oracle, scenes, name, fmt):
    """numpy = oracle = second reading, as the float32 means (sum / n in float) both restatements report; on the whole
    buffer and on a ragged head of it."""
    iq = scenes[name]
    of = {"sc16": oracle.FMT_SC16, "sc16q11": oracle.FMT_SC16Q11}[fmt]
    orc = oracle.Oracle(of, 58, 1, 0)
    for n in (len(iq), 77777, 1025):
        part = np.ascontiguousarray(iq[:n])
        sl, sp = S.sums(fmt, part)
        want = np.array([sl / F32(n), sp / F32(n)], dtype=F32)
        _, ol, op = orc.convert(part.view(np.uint8).reshape(-1), n)
        assert np.array_equal(S.bits(np.array([ol, op], dtype=F32)), S.bits(want)), (name, fmt, n, ol, op, want)
        assert float(F32(ol)) == ol and float(F32(op)) == op                              # the doubles hold float32 values
        _, lvl, pwr, float_sums = indep_demod.convert(fmt, part.tobytes(), False)
        assert float_sums
        il, ip = indep_demod.buffer_means(float_sums, lvl, pwr)
        assert np.array_equal(S.bits(np.array([il, ip], dtype=F32)), S.bits(want)), (name, fmt, n, il, ip, want)
    orc.close()


def test_magsq_reference_is_the_sc16_reference_on_the_squares(scenes):
    for name in S.NAMES:
        iq = scenes[name]
        assert np.array_equal(S.sums_bits("magsq", S.magsq_of(iq)), S.sums_bits("sc16", iq)), name
