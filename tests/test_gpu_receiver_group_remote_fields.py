"""msd_group_accept_beast_fields / msd_group_accept_avr_fields on the GPU.  Two groups of one configuration get the same
bytes, one through the plain accept call; the fields call must deliver the plain group's records, each with
msd_decode_fields(mm, NULL) -- struct bytes compared --, and leave the group in the plain call's state
(remote_out.Twin).  Every comparison is exact."""
import errno
import random

import numpy as np
import pytest

from remote_out import Twin, avr_stream, beast_stream, corpus, cut_at

pytestmark = pytest.mark.gpu


@pytest.fixture
def twin(pkg, torch_cuda):
    made = []

    def f(K, fields=True, **kw):
        flags = kw.pop("flags", 0) | (pkg.capi.CFG_DECODE_FIELDS if fields else 0)
        made.append(Twin(pkg, K, flags=flags, **kw))
        return made[-1]

    yield f
    for t in made:
        t.close()


def stream(kind, items, rng=None):
    return beast_stream(items, rng) if kind == "beast" else avr_stream(items, rng)


_parity = {}


# 1. parity: K = 4 at levels 0, 1, 2, 1, Mode A/C on for receiver 3, three calls cut inside frames and lines; the
# records hold every format the decoder knows
@pytest.mark.parametrize("stage", ["gpu", "host_resolve"])
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_parity(pkg, twin, kind, stage):
    K = 4
    T = twin(K, levels=[0, 1, 2, 1], modeac=[0, 0, 0, 1], flags=pkg.capi.CFG_HOST_RESOLVE if stage == "host_resolve" else 0)
    if kind not in _parity:  # once per input
        _parity[kind] = [stream(kind, corpus(random.Random(300 + r), 300), random.Random(400 + r)) for r in range(K)]
    data = _parity[kind]
    parts = [cut_at(data[r], (len(data[r]) // 3 + 5 + r, 2 * len(data[r]) // 3 + 11 + r)) for r in range(K)]
    dfs, metypes, commb, corrected = set(), {17: set(), 18: set()}, 0, set()
    for c in range(3):
        order = [(c + k) % K for k in range(K)]
        want, got = T.fields(kind, [(r, parts[r][c]) for r in order], 1000 + c, keep=True)
        for m in want:
            dfs.update(int(x) for x in m["msgtype"])
            corrected.update(int(x) for x in m["correctedbits"])
            for df in (17, 18):
                metypes[df].update(int(x[4]) >> 3 for x in m["msg"][m["msgtype"] == df])
            commb += int(np.isin(m["msgtype"], (20, 21)).sum())
    assert dfs >= {0, 4, 5, 11, 16, 17, 18, 20, 21, 32} and corrected == {0, 1, 2} and commb >= 10
    t = metypes[17]
    assert t & {1, 2, 3, 4} and t & {5, 6, 7, 8} and t & set(range(9, 19)) and t >= {19, 28, 29, 31} and metypes[18]
    T.same_state(random.Random(1), 2000)


# 2. Mode A/C: no carry between two consecutive replies -- the second one's altitude fields are its own
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_mode_ac_has_no_carry(pkg, twin, kind):
    T = twin(2, modeac=[1, 0])
    with_alt, ident = bytes([0x00, 0x40]), bytes([0x00, 0x80])  # a Mode C altitude; SPI set: no altitude of its own
    items = [(with_alt, 1, 0x40), (ident, 2, 0x40), (with_alt, 3, 0x40)]
    want, got = T.fields(kind, [(0, stream(kind, items)), (1, stream(kind, items))], 1)
    assert len(got[0]) == 3 and got[1] == []
    f = [ff for _, ff in got[0]]
    assert int(f[0]["altitude_baro_valid"]) == 1 and int(f[2]["altitude_baro_valid"]) == 1
    assert int(f[1]["altitude_baro_valid"]) == 0 and int(f[1]["altitude_baro"]) == 0 and int(f[1]["spi"]) == 1
    carried = pkg.capi.decode_fields(want[0][1], f[0])  # what a carry would have made of it
    assert int(carried["altitude_baro_valid"]) == 1 and int(carried["altitude_baro"]) == int(f[0]["altitude_baro"]) == -1200


# 3. a group without MSD_CFG_DECODE_FIELDS refuses, untouched; n == 0 calls no sink
@pytest.mark.parametrize("kind", ["beast", "avr"])
def test_arguments(pkg, twin, kind):
    items = corpus(random.Random(3), 60)
    F = stream(kind, items)
    T = twin(1, fields=False)
    want = T.records(T.plain, kind, [(0, F[:100])], 1)
    got = T.records(T.new, kind, [(0, F[:100])], 1)
    call = T.new.accept_beast_fields if kind == "beast" else T.new.accept_avr_fields
    with pytest.raises(pkg.capi.MsdError) as e:
        call([(0, F[100:])], 2)
    assert f"{-errno.EINVAL}" in str(e.value)
    a, b = T.records(T.plain, kind, [(0, F[100:])], 3), T.records(T.new, kind, [(0, F[100:])], 3)
    assert a[0].tobytes() == b[0].tobytes() and want[0].tobytes() == got[0].tobytes() and len(a[0]) > 10
    T.same_state(random.Random(3), 4)
    T2 = twin(2)
    call = T2.new.accept_beast_fields if kind == "beast" else T2.new.accept_avr_fields
    assert call([], 5) == {}
    with pytest.raises(pkg.capi.MsdError) as e:
        call([(0, F), (0, F)], 5)  # the same receiver twice
    assert f"{-errno.EINVAL}" in str(e.value)
    T2.fields(kind, [(1, F), (0, F[:50])], 6)
    T2.fields(kind, [(0, F[50:])], 7)
    T2.same_state(random.Random(3), 8)
