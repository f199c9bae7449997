"""The Mode A/C demodulator's exact comparisons reached on purpose: the constructed scenes of tests/ac_scenes.py through
Demodulator(fmt=FMT_MAG16, mode_ac=1), launch_device / launch_host, both resolve stages and batches of 1, 4 and 16
buffers, against the oracle's MAG16 replay (messages, counters, signal and noise power bit for bit) and against each
scene's designed answer.  Every compared quantity is an integer or a bit pattern."""
import numpy as np
import pytest

import ac_scenes as acs
from helpers import assert_same

pytestmark = pytest.mark.gpu

C = acs.CHUNK
SCENES = {"pulse-f1": ("pulse", "f1"), "pulse-f2": ("pulse", "f2"), "edge": ("edge",), "clock": ("clock",),
          "window": ("window",), "codes": ("codes",), "skip": ("skip",), "dense": ("dense",), "mixed": ("mixed",)}


@pytest.fixture(params=["gpu-resolve", "host-resolve"], autouse=True)
def resolve_stage(request, monkeypatch):
    monkeypatch.setenv("MSD_GPU_RESOLVE", "1" if request.param == "gpu-resolve" else "0")
    return request.param


_WANT = {}


def oracle_replay(oracle, key, sc):
    """The oracle's answer to a scene, computed once."""
    if key not in _WANT:
        _WANT[key] = oracle.Oracle(oracle.FMT_MAG16, 58, 1, 1).replay(sc.mag, cap=1 << 16)
    return _WANT[key]


def run(pkg, torch, mag, batch_bufs, via="device", **kw):
    """The capture through the pipelined stream interface in batches of batch_bufs buffers."""
    batch, n = batch_bufs * C, mag.size
    dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, nfix_crc=1, mode_ac=1, max_batch_samples=batch, message_capacity=1 << 16, **kw)
    if via == "device":
        d = torch.from_numpy(np.concatenate([mag, np.zeros(32, np.uint16)]).view(np.uint8)).to("cuda:0")
        return pkg.replay_device(dem, d.data_ptr(), n, batch), dem
    out, inflight, off, keep = [], 0, 0, []
    while True:
        m = min(batch, n - off)
        if inflight == pkg.capi.PIPELINE_DEPTH:
            out.append(dem.collect())
            inflight -= 1
            keep.pop(0)
        part = np.ascontiguousarray(mag[off:off + m]) if m else np.zeros(1, np.uint16)
        keep.append(part)   # alive until collected
        dem.launch_host(part, m, last=off + m >= n)
        inflight += 1
        off += m
        if off >= n:
            break
    while inflight:
        out.append(dem.collect())
        inflight -= 1
    return np.concatenate(out), dem


@pytest.mark.parametrize("via", ["device", "host"])
@pytest.mark.parametrize("batch_bufs", [1, 4, 16])
@pytest.mark.parametrize("name", list(SCENES))
def test_scene(pkg, oracle, torch_cuda, name, batch_bufs, via):
    """a: the pulse test at F1 (every residue mod 16, lanes 0 and 63) and at F2, one below, at and one above each bound;
    b: tile, buffer and capture edges; c: the clock of the first pulse; d: the bit windows at both thresholds; e: every
    code; f: the skip-ahead; g: dense and loud buffers (the unpacked F1 test, a second staging segment, rounds of more
    than 64 survivors, a silent buffer); i: Mode S frames beside the replies.  (tests/test_ac_scenes.py asserts the exact
    count of every designed outcome of every scene.)"""
    sc = acs.scene(*SCENES[name])
    want, wstats = oracle_replay(oracle, name, sc)
    got, dem = run(pkg, torch_cuda, sc.mag, batch_bufs, via)
    assert_same(got, dem.stats(), want, wstats)
    exp = sc.expected()
    acs.check_replies(got, exp)
    assert dem.stats()["demod_modeac"] == exp["demod_modeac"] > 0
    if sc.designed:   # both sides of the scene's bounds occurred, reply by reply
        delivered = {(int(m["timestampMsg"]), (int(m["msg"][0]) << 8) | int(m["msg"][1])) for m in got[got["msgtype"] == 32]}
        kept = [r for r in sc.replies if r["expect"] == acs.DELIVERED]
        assert len(kept) == len(delivered) and all((r["ts"], r["code"]) in delivered for r in kept)
        twins = {(r["ts"], r["code"]) for r in kept}   # (a shoulder pair: the position beside a rejected one reads the same reply)
        gone = [r for r in sc.replies if r["expect"] not in (acs.DELIVERED, acs.HIDDEN) and (r["ts"], r["code"]) not in twins]
        assert name in ("clock", "codes", "mixed") or len(gone) >= 2
        assert not any((r["ts"], r["code"]) in delivered for r in gone)


def test_every_code_with_decoded_fields(pkg, oracle, torch_cuda):
    """Scene e once more with decode_fields: every Mode C altitude and every identity through the emit kernel (or, with
    the host resolve stage, the same code on the host), against oracle.replay_fields."""
    from test_fields import FIELD_NAMES
    sc = acs.scene("codes")
    dem = pkg.Demodulator(fmt=pkg.FMT_MAG16, nfix_crc=1, mode_ac=1, max_batch_samples=8 * C, message_capacity=1 << 16,
                          decode_fields=True)
    d = torch_cuda.from_numpy(np.concatenate([sc.mag, np.zeros(32, np.uint16)]).view(np.uint8)).to("cuda:0")
    msgs, fields = [], []
    for off in range(0, sc.n, 8 * C):
        m = min(8 * C, sc.n - off)
        dem.launch_device(d.data_ptr() + 2 * off, m, off + m >= sc.n)
        mm, ff = dem.collect_fields()
        msgs.append(mm)
        fields.append(ff)
    msgs, fields = np.concatenate(msgs), np.concatenate(fields)
    want, wfields, wstats = oracle.Oracle(oracle.FMT_MAG16, 58, 1, 1).replay_fields(sc.mag, cap=1 << 16)
    assert_same(msgs, dem.stats(), want, wstats)
    for f in FIELD_NAMES:
        assert np.array_equal(fields[f], wfields[f]), f
    acs.check_replies(msgs, sc.expected())
    assert len(msgs) == 8192 and (fields["altitude_baro_valid"] == 1).sum() > 1000


@pytest.mark.parametrize("tiles_per_wave", [2, 3])
def test_more_than_one_tile_per_wavefront(pkg, oracle, torch_cuda, tiles_per_wave):
    """Scene h: one batch with more tiles than the candidate kernel has regions (28 per CU), so that a wavefront owns 2
    or 3 tiles: the tile-to-tile prefetch, the fast load of tiles inside the batch, and the per-wave noise level, which
    with 3 tiles (128 tiles a buffer) changes buffer inside a wavefront.  Every buffer has a reply exactly at its own
    level bound and one a unit below, in its first and in its last tile."""
    regions = 28 * torch_cuda.cuda.get_device_properties(0).multi_processor_count
    tiles = C // acs.TILE
    nb = (tiles_per_wave - 1) * regions // tiles + 1
    assert -(-nb * tiles // regions) == tiles_per_wave and nb * C <= 1 << 28
    sc = acs.scene("waves", nb)
    want, wstats = oracle_replay(oracle, ("waves", nb), sc)
    got, dem = run(pkg, torch_cuda, sc.mag, nb)
    assert_same(got, dem.stats(), want, wstats)
    acs.check_replies(got, sc.expected())
    assert sc.count("f1") == 2 * nb and dem.stats()["demod_modeac"] == len(sc.replies) - 2 * nb
