"""The float-sum kernels alone (msd_fm_totals_kernel, msd_fm_functions_kernel, msd_fm_apply_kernel and the
one-wavefront-per-sum msd_float_means_kernel) on the constructed buffers of tests/fm_scenes.py, driven through the entries
libmodes_hip.so exports (msd_launch_float_means, msd_launch_dc_sums, msd_fm_work_bytes, msd_fm_deferrable), against the
numpy reference of fm_scenes.py.  Every comparison is bit equality of float32: there is no tolerance anywhere.

What the scenes reach that noise does not: more edge blocks than a sum has slots for sub-block functions (FM_SLOTS), sums
that stagnate or tie in every addition, sums below the e >= -7 floor for a whole buffer, landings exactly on a power of
two, a binade left inside one lane's sixteen elements -- and predictions (tile_sums) that are wrong on purpose: DESIGN.md
4.4 claims the result is the sequential sum "whatever the predictions".  Every launch here is an ordinary launch on valid
memory."""
import ctypes as C

import numpy as np
import pytest

import fm_scenes as S
from helpers import assert_same, fmt_ids

pytestmark = pytest.mark.gpu

BUF, BLK, NBLK = S.BUF, S.BLK, S.NBLK
OVERHANG = 5000                     # samples behind a buffer that the "long" entry takes along
FORMATS = S.FORMATS
IQ_FORMATS = ("sc16", "sc16q11")
ENTRIES = ("phase0", "phase1-then-2", "no-work", "long")
LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 65536, 131071, 131072)
LENGTH_CONTENTS = ("noise-0.3", "saturated-max-min", "stagnate-a384")


class Fm:
    """The library's entries, every scene on the device (per format, consecutive buffers, the first scene's head once more
    behind the last) and the reference sums."""

    def __init__(self, pkg, torch):
        self.torch = torch
        L = C.CDLL(pkg.capi.LIB_PATH)
        L.msd_fm_work_bytes.restype = C.c_size_t
        L.msd_fm_work_bytes.argtypes = [C.c_uint32]
        L.msd_fm_deferrable.restype = C.c_int
        L.msd_fm_deferrable.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
        L.msd_launch_float_means.restype = C.c_int
        L.msd_launch_float_means.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p]
        L.msd_launch_dc_sums.restype = C.c_int
        L.msd_launch_dc_sums.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p]
        self.L = L
        self.fid = {"sc16": pkg.FMT_SC16, "sc16q11": pkg.FMT_SC16Q11}
        self.names = S.NAMES
        self.index = {n: i for i, n in enumerate(self.names)}
        scenes = [S.make(n) for n in self.names]
        assert all(len(s) == BUF for s in scenes)
        iq = np.concatenate(scenes + [scenes[0][:OVERHANG]])
        self.host = {"sc16": iq, "sc16q11": iq, "magsq": S.magsq_of(iq)}   # 4 bytes per sample in every format
        self.dev = {"magsq": torch.from_numpy(self.host["magsq"]).cuda()}
        self.dev["sc16"] = self.dev["sc16q11"] = torch.from_numpy(iq).cuda()
        self.want = {f: np.stack([S.sums_bits(f, self.part(f, i * BUF, BUF)) for i in range(len(scenes))]) for f in FORMATS}
        self.totals = {f: np.stack([S.block_totals(f, self.part(f, i * BUF, BUF)) for i in range(len(scenes))])
                       for f in IQ_FORMATS}
        self.work1 = self.work(1)

    def part(self, fmt, first, n):
        return self.host[fmt][first: first + n]

    def ptr(self, fmt, first=0):
        return self.dev[fmt].data_ptr() + 4 * first

    def upload(self, fmt, host):
        """a device allocation of exactly these samples"""
        return self.torch.from_numpy(np.ascontiguousarray(host)).cuda()

    def work(self, nbuffers):
        return self.torch.zeros(self.L.msd_fm_work_bytes(nbuffers), dtype=self.torch.uint8, device="cuda")

    def deferrable(self, work, buffer_len, nbuffers):
        return self.L.msd_fm_deferrable(work.data_ptr() if work is not None else None, buffer_len, nbuffers)

    def run(self, fmt, ptr, nsamples, buffer_len, nbuffers, work=None, tile=None, phases=(0,)):
        """-> the [nbuffers][level, power] sums as uint32 bits; the output starts as NaNs, so a sum not written shows"""
        t = self.torch
        out = t.full((nbuffers, 2), float("nan"), dtype=t.float32, device="cuda")
        d_tile = t.from_numpy(np.ascontiguousarray(tile, dtype=np.float32)).cuda() if tile is not None else None
        wp = work.data_ptr() if work is not None else None
        for phase in phases:
            if fmt == "magsq":
                assert tile is None                     # msd_launch_dc_sums has no tile sums: its totals kernel runs
                rc = self.L.msd_launch_dc_sums(ptr, nsamples, buffer_len, nbuffers, out.data_ptr(), wp, phase, None)
            else:
                rc = self.L.msd_launch_float_means(self.fid[fmt], ptr, nsamples, buffer_len, nbuffers, out.data_ptr(),
                                                   d_tile.data_ptr() if d_tile is not None else None, wp, phase, None)
            assert rc == 0, (fmt, phase, rc)
        t.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)


def same(got, want, where):
    got, want = np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        b, j = (int(v) for v in bad[0])
        raise AssertionError(f"{where}: {len(bad)} sums differ, first: buffer {b} {'level' if j == 0 else 'power'} sum "
                             f"{got.view(np.float32)[b, j]!r} ({int(got[b, j]):#010x}) != "
                             f"{want.view(np.float32)[b, j]!r} ({int(want[b, j]):#010x})")


@pytest.fixture(scope="module")
def fm(pkg, torch_cuda):
    return Fm(pkg, torch_cuda)


# ---------------------------------------------------------------------------------------------------------------------
# every scene, format and entry
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", S.NAMES)
def test_scene(fm, name, fmt, entry):
    i = fm.index[name]
    first = i * BUF
    if entry == "long":
        # one buffer longer than 131072 samples, buffer_len = nsamples, as the converter entry calls: the three kernels
        # do not take it (msd_fm_deferrable says so), the one-wavefront-per-sum kernel does
        n = BUF + OVERHANG
        assert fm.deferrable(fm.work1, n, 1) == 0
        got = fm.run(fmt, fm.ptr(fmt, first), n, n, 1, work=fm.work1)
        same(got, [S.sums_bits(fmt, fm.part(fmt, first, n))], (name, fmt, entry))
        return
    assert fm.deferrable(fm.work1, BUF, 1) == 1 and fm.deferrable(None, BUF, 1) == 0
    if entry == "phase0":
        got = fm.run(fmt, fm.ptr(fmt, first), BUF, BUF, 1, work=fm.work1)
    elif entry == "phase1-then-2":
        got = fm.run(fmt, fm.ptr(fmt, first), BUF, BUF, 1, work=fm.work1, phases=(1, 2))
    else:
        got = fm.run(fmt, fm.ptr(fmt, first), BUF, BUF, 1, work=None)
    same(got, fm.want[fmt][i: i + 1], (name, fmt, entry))


# ---------------------------------------------------------------------------------------------------------------------
# predictions wrong on purpose
# ---------------------------------------------------------------------------------------------------------------------

def wrong_totals(fm, fmt, i, kind):
    """[NBLK][level, power] float32 in place of the scan's tile sums.  Finite and non-negative throughout: that is what
    the scan can leave (sums of magnitudes and of squares), and all the kernels are asked to stand."""
    honest = fm.totals[fmt][i]
    rng = np.random.default_rng(1000 + i)
    if kind == "honest":
        t = honest
    elif kind == "zeros":
        t = np.zeros_like(honest)
    elif kind == "doubled":
        t = honest * np.float32(2.0)
    elif kind == "halved":
        t = honest * np.float32(0.5)
    elif kind == "neighbour":
        t = fm.totals[fmt][(i + 1) % len(fm.names)]
    elif kind == "shifted-one-block":
        t = np.roll(honest, 1, axis=0)
        t[0] = 0
    elif kind == "random-to-2^20":
        t = (rng.random(honest.shape) * 2.0 ** 20).astype(np.float32)
    elif kind == "random-magnitudes":
        t = (2.0 ** rng.uniform(-40.0, 20.0, honest.shape)).astype(np.float32)
    elif kind == "all-2^20":
        t = np.full_like(honest, 2.0 ** 20)
    else:
        raise ValueError(kind)
    t = np.ascontiguousarray(t, dtype=np.float32)
    assert np.isfinite(t).all() and (t >= 0).all() and not np.signbit(t).any() and t.max() <= 2.0 ** 20
    return t


PREDICTIONS = ("honest", "zeros", "doubled", "halved", "neighbour", "shifted-one-block", "random-to-2^20",
               "random-magnitudes", "all-2^20")


@pytest.mark.parametrize("kind", PREDICTIONS)
@pytest.mark.parametrize("fmt", IQ_FORMATS)
@pytest.mark.parametrize("name", S.NAMES)
def test_scene_whatever_the_predictions(fm, name, fmt, kind):
    """tile_sums given (buffer_len = 131072, so they are used): the sums must not change by one bit."""
    i = fm.index[name]
    tile = wrong_totals(fm, fmt, i, kind)
    got = fm.run(fmt, fm.ptr(fmt, i * BUF), BUF, BUF, 1, work=fm.work1, tile=tile)
    same(got, fm.want[fmt][i: i + 1], (name, fmt, kind))


# ---------------------------------------------------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", LENGTH_CONTENTS)
def test_one_buffer_of_n_samples(fm, name, fmt, n):
    """The first n samples of a scene in an allocation of exactly n samples: as the ragged last buffer of a batch
    (buffer_len = 131072), as the converter entry calls (buffer_len = n), and through the one-wavefront-per-sum kernel."""
    host = fm.part(fmt, fm.index[name] * BUF, n)
    want = [S.sums_bits(fmt, host)]
    d = fm.upload(fmt, host)
    assert fm.deferrable(fm.work1, n, 1) == 1
    same(fm.run(fmt, d.data_ptr(), n, BUF, 1, work=fm.work1), want, (name, fmt, n, "buffer_len 131072"))
    same(fm.run(fmt, d.data_ptr(), n, n, 1, work=fm.work1), want, (name, fmt, n, "buffer_len n"))
    same(fm.run(fmt, d.data_ptr(), n, n, 1, work=fm.work1, phases=(1, 2)), want, (name, fmt, n, "buffer_len n, two phases"))
    same(fm.run(fmt, d.data_ptr(), n, n, 1, work=None), want, (name, fmt, n, "no work"))


@pytest.mark.parametrize("with_work", [True, False], ids=["work", "no-work"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["stagnate-a384", "one-large-block63-offset17", "noise-0.05", "quiet-loud-alternating"])
def test_batch_with_a_ragged_last_buffer(fm, name, fmt, with_work):
    i = min(fm.index[name], len(fm.names) - 3)
    ragged = 77777
    n = 2 * BUF + ragged
    host = fm.part(fmt, i * BUF, n)
    want = np.stack([fm.want[fmt][i], fm.want[fmt][i + 1], S.sums_bits(fmt, host[2 * BUF:])])
    d = fm.upload(fmt, host)
    got = fm.run(fmt, d.data_ptr(), n, BUF, 3, work=fm.work(3) if with_work else None)
    same(got, want, (name, fmt, with_work))
    if with_work and fmt != "magsq":
        tile = np.concatenate([fm.totals[fmt][i], fm.totals[fmt][i + 1], S.block_totals(fmt, host[2 * BUF:])])
        same(fm.run(fmt, d.data_ptr(), n, BUF, 3, work=fm.work(3), tile=tile), want, (name, fmt, "tile sums"))


@pytest.mark.parametrize("entry", ["phase0", "phase1-then-2", "no-work", "tile-sums"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_empty_buffer_behind_an_exact_multiple(fm, fmt, entry):
    """nsamples = 2 * 131072 and nbuffers = 3, the allocation exactly nsamples: the third buffer reports 0.0 and has no
    samples to read."""
    if entry == "tile-sums" and fmt == "magsq":
        entry = "phase0"            # msd_launch_dc_sums takes none
    i = fm.index["stagnate-a256"]
    d = fm.upload(fmt, fm.part(fmt, i * BUF, 2 * BUF))
    want = np.concatenate([fm.want[fmt][i: i + 2], np.zeros((1, 2), dtype=np.uint32)])
    kw = {"phase0": dict(work=fm.work(3)), "phase1-then-2": dict(work=fm.work(3), phases=(1, 2)), "no-work": dict(work=None),
          "tile-sums": dict(work=fm.work(3), tile=fm.totals[fmt][i: i + 2].reshape(-1, 2) if fmt != "magsq" else None)}[entry]
    same(fm.run(fmt, d.data_ptr(), 2 * BUF, BUF, 3, **kw), want, (fmt, entry))


# ---------------------------------------------------------------------------------------------------------------------
# many buffers in one launch, and a work area that is used again
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_all_scenes_in_one_launch_and_the_work_area_reused(fm, fmt):
    """All scenes as consecutive buffers of one launch (every buffer its own FmBufWork), in two orders; the second launch
    uses the first one's work area as it was left: functions, slots and sub-block functions of the launch before must not
    be picked up.  Then the first order again in two phases, over what the second left."""
    k = len(fm.names)
    work = fm.work(k)
    tile = fm.totals[fmt].reshape(-1, 2) if fmt != "magsq" else None
    same(fm.run(fmt, fm.ptr(fmt), k * BUF, BUF, k, work=work, tile=tile), fm.want[fmt], (fmt, "in order"))
    perm = np.random.default_rng(2024).permutation(k)
    assert (perm != np.arange(k)).sum() > k // 2
    host = np.concatenate([fm.part(fmt, int(i) * BUF, BUF) for i in perm])
    d = fm.upload(fmt, host)
    same(fm.run(fmt, d.data_ptr(), k * BUF, BUF, k, work=work), fm.want[fmt][perm], (fmt, "permuted, work reused"))
    same(fm.run(fmt, fm.ptr(fmt), k * BUF, BUF, k, work=work, phases=(1, 2)), fm.want[fmt], (fmt, "in order again, two phases"))
    rev = np.arange(k)[::-1]
    host = np.concatenate([fm.part(fmt, int(i) * BUF, BUF) for i in rev])
    d = fm.upload(fmt, host)
    if tile is not None:
        tile = fm.totals[fmt][rev].reshape(-1, 2)
    same(fm.run(fmt, d.data_ptr(), k * BUF, BUF, k, work=work, tile=tile), fm.want[fmt][rev], (fmt, "reversed, work reused"))
    same(fm.run(fmt, d.data_ptr(), k * BUF, BUF, k, work=None), fm.want[fmt][rev], (fmt, "reversed, no work"))


# ---------------------------------------------------------------------------------------------------------------------
# through the product: the scan's real tile sums and the pipeline's deferred apply walk in the loop
# ---------------------------------------------------------------------------------------------------------------------

_oracle_runs = {}


def product_capture(pkg, f):
    """every scene, then two buffers and a ragged one of generated traffic (Mode S and Mode A/C replies), so that the
    message lists and counters compared are not empty"""
    n_tail = 2 * BUF + 4321
    tail = pkg.siggen.generate(pkg.siggen.make_cfg(seed=77, fmt=f, msgs_per_sec=5000, n_aircraft=20, ac_per_sec=400), n_tail)
    iq = np.concatenate([S.make(n).reshape(-1).view(np.uint8) for n in S.NAMES] + [np.asarray(tail).view(np.uint8).reshape(-1)])
    return iq, len(S.NAMES) * BUF + n_tail


@pytest.mark.parametrize("way", ["single-batch", "pipelined"])
@pytest.mark.parametrize("fmt,mode_ac,dc", [("sc16", 0, False), ("sc16q11", 0, False), ("sc16", 0, True),
                                            ("sc16", 1, False)],
                         ids=["sc16", "sc16q11", "sc16-dcfilter", "sc16-modeac"])
def test_scenes_through_the_demodulator(pkg, oracle, torch_cuda, fmt, mode_ac, dc, way):
    """All scenes concatenated into one capture (generated traffic and a ragged buffer last): buffer_means() equal to the oracle's bit for
    bit, messages and counters equal; with Mode A/C on once, the consumer of the means (demodulate2400AC's noise level)."""
    f, of = fmt_ids(pkg, oracle, fmt)
    iq, n = product_capture(pkg, f)
    key = (fmt, mode_ac, dc)
    if key not in _oracle_runs:
        _oracle_runs[key] = oracle.Oracle(of, 58, 1, mode_ac, dc_filter=dc).replay(iq, cap=1 << 18, want_means=True)
    want, wstats, wmeans = _oracle_runs[key]
    nbuf = len(S.NAMES) + 3
    assert wstats["buffers"] == nbuf and len(want) > 50 and (wstats["demod_modeac"] > 0) == bool(mode_ac)
    d_iq = torch_cuda.from_numpy(iq).to("cuda:0")
    batch = n if way == "single-batch" else 4 * BUF
    dem = pkg.Demodulator(fmt=f, nfix_crc=1, mode_ac=mode_ac, max_batch_samples=batch, message_capacity=1 << 18, dc_filter=dc)
    got, means, inflight, off = [], [], 0, 0

    def collect_one():
        got.append(dem.collect())
        means.append(dem.buffer_means())

    while off < n:
        if inflight == pkg.capi.PIPELINE_DEPTH:
            collect_one()
            inflight -= 1
        m = min(batch, n - off)
        dem.launch_device(d_iq.data_ptr() + 4 * off, m, last=off + m >= n)
        inflight += 1
        off += m
    while inflight:
        collect_one()
        inflight -= 1
    gm = np.concatenate(means)
    assert len(gm) == nbuf
    assert np.array_equal(gm.view(np.uint64), wmeans[:nbuf].view(np.uint64)), \
        (key, way, [(int(b), gm[b].tolist(), wmeans[b].tolist()) for b in np.flatnonzero((gm != wmeans[:nbuf]).any(axis=1))[:8]])
    assert_same(np.concatenate(got), dem.stats(), want, wstats)
    dem.close()
