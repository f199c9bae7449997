"""CRC repair on the GPU with every one- and two-bit error pattern, once (tests/repair_scenes.py): step C of the scan kernel
(the bucketed single-bit syndromes in LDS, --aggressive's hash table in global memory, the DF11 mask, the address-bit
repair) and both resolve stages through the stream interface; the receiver-group instantiation with a repair level per
receiver; and the Beast input's copy of the lookups.  Every run is held to the oracle (or, for Beast input, the checker
of tests/remote_decode.py) message for message, and to the scene's designed answer."""
import random

import numpy as np
import pytest

import mag_scenes as ms
import repair_scenes as rs
from helpers import assert_same, assert_same_stats
from remote_decode import Checker, assert_same_records, assert_same_stats as assert_same_remote_stats, frame
from test_gpu_beast_ingest import probe, random_chunks, remote
from test_gpu_mag_scenes import oracle_replay, run
from test_gpu_receiver_group import OracleReceiver, group_flags, same
from test_gpu_receiver_group_beast import Rig

pytestmark = pytest.mark.gpu

C = ms.CHUNK
SCENES = {"long": rs.long_scene, "short": rs.short_scene}


# ---- the stream interface, magnitudes in ----------------------------------------------------------------------------------

@pytest.fixture(params=["gpu-resolve", "host-resolve"])
def resolve_stage(request, monkeypatch):
    monkeypatch.setenv("MSD_GPU_RESOLVE", "1" if request.param == "gpu-resolve" else "0")
    return request.param


_WANT = {}


def oracle_mag16(oracle, name, nfix):
    """The oracle's replay of a scene at a level, made once and left alone."""
    if (name, nfix) not in _WANT:
        _WANT[name, nfix] = oracle_replay(oracle, SCENES[name]().mag, 58, nfix)[:2]
    return _WANT[name, nfix]


CASES = [(name, nfix, 4) for name in sorted(SCENES) for nfix in (0, 1, 2)] + [("long", 2, 1), ("long", 2, 16)]


@pytest.mark.parametrize("name,nfix,batch_bufs", CASES)
def test_every_pattern_through_scan_and_resolve(pkg, oracle, torch_cuda, resolve_stage, name, nfix, batch_bufs):
    """Every frame of the scene decided as designed: which patterns are repaired at this level, to which bytes, which of
    them the address filter lets through; position, phase and the preamble counters besides."""
    sc = rs.design(SCENES[name](), nfix)
    want, wstats = oracle_mag16(oracle, name, nfix)
    got, dem = run(pkg, torch_cuda, sc.mag, nfix=nfix, batch_bufs=batch_bufs)
    gstats = dem.stats()
    dem.close()
    assert_same(got, gstats, want, wstats)
    exp = sc.expected(58)
    ms.check_frames(got, exp["frames"])
    ms.check_counts(gstats, exp)
    assert got["correctedbits"].tolist() == [f["corrected"] for f in exp["frames"]]
    assert list(gstats["demod_accepted"]) == rs.histogram(sc)


# ---- receiver groups, the UC8 rendering -----------------------------------------------------------------------------------

_GROUP_WANT = {}


def oracle_uc8_live(oracle, name, level):
    """One live receiver of the oracle at a level fed the scene's UC8 buffers: (messages per buffer, counters), once."""
    if (name, level) not in _GROUP_WANT:
        iq = rs.to_uc8(SCENES[name]())
        ref = OracleReceiver(oracle, oracle.FMT_UC8, level)
        outs = [ref.feed(iq[2 * C * b:2 * C * (b + 1)]) for b in range(iq.size // (2 * C))]
        _GROUP_WANT[name, level] = outs, ref.stats()
    return _GROUP_WANT[name, level]


@pytest.mark.parametrize("stage", [0, "host_resolve"])
@pytest.mark.parametrize("levels", [(0, 1), (0, 1, 2, 1, 0, 2)], ids=["levels-0-1", "levels-0-1-2-1-0-2"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_receiver_group_with_a_level_per_receiver(pkg, oracle, torch_cuda, name, levels, stage):
    """Every receiver of a group is fed the same buffers, one per call.  Levels (0, 1): the scan without the two-bit
    tables, the bucket lookup gated by the receiver's level.  Levels (0, 1, 2, 1, 0, 2): the FIX2 scan with all three
    branches in one launch.  Each receiver delivers what the oracle of its level delivers, and the designed messages."""
    sc = SCENES[name]()
    iq = rs.to_uc8(sc)
    K = len(levels)
    g = pkg.capi.ReceiverGroup(K, fmt=pkg.capi.FMT_UC8, nfix_crc=0, flags=group_flags(pkg, stage))
    try:
        for r, level in enumerate(levels):
            g.set_receiver_options(r, nfix_crc=level)
        got = [[] for _ in range(K)]
        for b in range(iq.size // (2 * C)):
            out = g.submit(np.tile(iq[2 * C * b:2 * C * (b + 1)], K), list(range(K)))
            for r, level in enumerate(levels):
                mine = out["m"][out["receiver"] == r]
                same(mine, oracle_uc8_live(oracle, name, level)[0][b], f"buffer {b} receiver {r} level {level}")
                got[r].append(mine)
        for r, level in enumerate(levels):
            assert_same_stats(g.stats(r), oracle_uc8_live(oracle, name, level)[1])
            rs.check_uc8(np.concatenate(got[r]), rs.design(sc, level))
            assert list(g.stats(r)["demod_accepted"])[level + 1:] == [0] * (2 - level)
    finally:
        g.close()


# ---- Beast input ----------------------------------------------------------------------------------------------------------

def beast_plan(nfix):
    """(the clean frames of A, every other frame of both scenes) in the order they are sent, designed for Beast input at
    this level through one filter."""
    lng, sht = rs.long_scene().frames, rs.short_scene().frames
    first, rest = [lng[0], sht[0]], lng[1:] + sht[1:]
    rs.design_frames(first + rest, nfix, demod=False)
    return first, rest


def beast_bytes(frames):
    return b"".join(frame(ord("3") if f["msgbits"] == 112 else ord("2"), f["rx"]) for f in frames)


def designed(frames):
    return [(f["bytes"], f["corrected"]) for f in frames if f["accept"]]


def delivered(records):
    return [(bytes(m["msg"][: int(m["msgbits"]) // 8]), int(m["correctedbits"])) for m in records]


@pytest.mark.parametrize("nfix", [0, 1, 2])
def test_every_pattern_as_beast_input(pkg, oracle, torch_cuda, nfix):
    """The received bytes of every frame as Beast frames through msd_accept_beast (diagnose / decide of the frames
    path): A's clean frames in a call of their own, then every pattern in random chunks."""
    first, rest = beast_plan(nfix)
    rng = random.Random(20 + nfix)
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=nfix, message_capacity=1 << 20, max_batch_samples=4 * C)
    chk = Checker(pkg, oracle, nfix, 0)
    try:
        head = dem.accept_beast(beast_bytes(first), 5)
        assert_same_records(head, chk.beast(beast_bytes(first), 5))
        assert delivered(head) == designed(first) and len(head) == 2
        data, pos, got = beast_bytes(rest), 0, []
        for k in random_chunks(rng, len(data)):
            part = data[pos:pos + k]
            pos += k
            got.append(dem.accept_beast(part, 6))
            assert_same_records(got[-1], chk.beast(part, 6))
        assert_same_remote_stats(remote(dem), chk.stats)
        assert delivered(np.concatenate(got)) == designed(rest)
        assert chk.stats["remote_accepted"][nfix] > 0
        probe(dem, chk, 7, rng)
    finally:
        dem.close()


def test_every_pattern_as_beast_input_of_a_group(pkg, oracle, torch_cuda):
    """The same bytes to three receivers of a group at levels 0, 1 and 2, in the same chunks of one call each."""
    levels = [0, 1, 2]
    R = Rig(pkg, oracle, 3, nfix=0, levels=levels)
    rng = random.Random(31)
    try:
        first, rest = beast_plan(0)
        head, data = beast_bytes(first), beast_bytes(rest)
        R.call([(r, head) for r in range(3)], 5)
        got, pos = [[] for _ in levels], 0
        for k in random_chunks(rng, len(data)):
            out = R.call([(r, data[pos:pos + k]) for r in range(3)], 6)
            pos += k
            for r in range(3):
                got[r].append(out[r])
        R.check_stats()
        for r, level in enumerate(levels):
            first, rest = beast_plan(level)
            assert delivered(np.concatenate(got[r])) == designed(rest), level
        R.probe(7, rng)
    finally:
        R.close()
