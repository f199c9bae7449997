"""Constructed u16 magnitude buffers (MSD_FMT_MAG16 input) with a designed answer: plain numpy, no product or oracle code.

Every decision of demodulate2400 (demod_2400.c:236-428) is an exact integer comparison, and random captures reach its
bounds only by chance.  A scene places every pulse at an exact sample and an exact level instead:

  * Mode S frames (indep_signal.mode_s_frame / crc24): DF, address, payload, flipped bits, rendered on the 12 MHz grid
    (five ticks per sample) at a chosen start sample and sub-sample tick, box-averaged to the sample grid, with exact
    high / low levels up to 65535.  The tick selects the trial phase that slices the frame: a frame that starts at tick
    T is read by position j with phase tp where 5 j + tp = T + 1 (data bit k at tick 95 + tp + 12 k of position j,
    SURVEY.md 8 a8, and 96 ticks of preamble).  A box-averaged pulse on a zero floor slices the same from tick T - 2
    to T and sometimes a little later (the correlators of demod_2400.c:73-93 see the same signs), so every trial phase
    reading it there scores alike: the first one scanned wins (the earlier position; at one position the lowest
    phase), and the designed reading is T - 2.  Two or three phases of one position tie whenever T - 2 and T share a
    position.  (The tolerance is the builder's model, checked against the oracle by tests/test_mag_scenes.py);
  * bare preamble windows, where each of the three pre-check comparisons and each of the three threshold tests is put
    a chosen distance (-1: one below, 0: equal, +1: one above, or far) from its bound.

A scene's `expected(threshold)` is its own answer: the frames it placed, and how many positions pass the pre-check and
each threshold test, counted by a vectorised restatement of the six comparisons over every scan position of the
capture, with the skip-ahead of the frames it expects to be accepted.  The oracle is the second answer.
"""
import numpy as np

import indep_signal

CHUNK = 131072
OVERLAP = 326
TICKS = indep_signal.TICKS


def frame_bits(rng, df, addr, flip=(), parity_xor=0, body=None):
    """The bits of one frame.  parity_xor: xored onto the 24 parity bits (DF11 with IID != 0: the IID); body: the
    data bits in front of the parity (DF and address included) instead of random ones."""
    if body is None:
        bits = indep_signal.mode_s_frame(rng, df, addr)
    else:
        body = np.asarray(body, dtype=np.uint8)
        parity = indep_signal.crc24(body) ^ (0 if df in (11, 17, 18) else addr)
        bits = np.concatenate([body, indep_signal.to_bits(parity, 24)])
    bits = bits.copy()
    bits[-24:] ^= indep_signal.to_bits(parity_xor, 24)
    for f in flip:
        bits[f] ^= 1
    return bits


def bits_to_bytes(bits):
    return np.packbits(np.asarray(bits, dtype=np.uint8)).tobytes()


def detection(tick):
    """(position j, trial phase tp) that slices a frame starting at 12 MHz tick `tick`: 5 j + tp = tick + 1, 4 <= tp <= 8."""
    for tp in range(4, 9):
        if (tick + 1 - tp) % TICKS == 0:
            return (tick + 1 - tp) // TICKS, tp
    raise AssertionError


def preamble_verdicts(z, threshold):
    """The six comparisons of demod_2400.c:276-307 at every position j of the magnitude array z with j + 19 < len(z):
    (pre-check, test 4/5, test 6/7, test 8) as boolean arrays."""
    z = np.asarray(z, dtype=np.int64)
    n = z.size - 19
    if n <= 0:
        return [np.zeros(0, bool)] * 4
    pa = [z[d:d + n] for d in range(19)]
    pre = (pa[1] > pa[7]) & (pa[12] > pa[14]) & (pa[12] > pa[15])
    ref = ((pa[5] + pa[8] + pa[16] + pa[17] + pa[18]) * threshold) >> 5
    d23, d1011 = pa[2] - pa[3], pa[10] - pa[11]
    common = pa[1] + pa[4] - d23 + pa[9] + pa[12]
    return pre, common - d1011 >= ref, common + d1011 >= ref, pa[1] + pa[4] + 2 * d23 + d1011 + pa[12] >= ref


class Scene:
    """A capture of n u16 magnitudes on a flat background."""

    def __init__(self, n, background=0, seed=0):
        self.mag = np.full(n, background, dtype=np.uint16)
        self.rng = np.random.default_rng(seed)
        self.frames = []      # dicts: sample, tick, j, phase, df, addr, bits, bytes, accept
        self.windows = []     # dicts: j, pre, tests (the designed margins), values

    @property
    def n(self):
        return self.mag.size

    def _put(self, start, values):
        lo, hi = max(start, 0), min(start + values.size, self.n)
        if hi > lo:
            self.mag[lo:hi] = np.maximum(self.mag[lo:hi], values[lo - start:hi - start])

    def frame(self, sample, sub=0, df=17, addr=0x4840D6, high=20000, low=0, flip=(), parity_xor=0, body=None,
              accept=True, bits=None):
        """A Mode S frame starting sub ticks (0..4) into `sample`; each sample is low + (high - low) * (ticks of the
        pulse in it) // 5.  accept: whether the scene expects it to be accepted (the skip-ahead of expected())."""
        if bits is None:
            clean = frame_bits(self.rng, df, addr, (), parity_xor, body)
        else:
            clean = np.asarray(bits, dtype=np.uint8)
        bits = clean.copy()
        for k in flip:
            bits[k] ^= 1
        env = indep_signal.mode_s_envelope(bits)
        tick = TICKS * sample + sub
        lead = tick % TICKS
        grid = np.zeros(lead + env.size + TICKS, dtype=np.int64)
        grid[lead:lead + env.size] = env.astype(np.int64)
        cnt = grid[: (grid.size // TICKS) * TICKS].reshape(-1, TICKS).sum(axis=1)
        vals = (low + (high - low) * cnt // TICKS).astype(np.uint16)
        self._put(tick // TICKS, vals)
        j, tp = detection(tick - 2)   # on a zero floor the slicer reads the frame from two ticks early (module doc)
        f = dict(sample=sample, tick=tick, j=j, phase=tp, df=int(bits[:5].dot(1 << np.arange(4, -1, -1))), addr=addr,
                 bits=bits, bytes=bits_to_bytes(clean), msgbits=len(bits), accept=accept, flips=len(flip))
        self.frames.append(f)
        return f

    def preamble(self, j, threshold, pre=(1, 1, 1), tests=(0, 0, 0), base=(100, 100, 100, 100, 100), d23=None):
        """A bare preamble window at position j (samples j .. j + 18): pa[1] - pa[7], pa[12] - pa[14], pa[12] - pa[15]
        are pre[0..2], and each threshold test's left side minus ref_level = (base_noise * threshold) >> 5 is
        tests[0..2] (tests[1] - tests[0] must be even: the two differ by 2 (pa[10] - pa[11])).  base: pa[5], pa[8],
        pa[16], pa[17], pa[18].  Every other sample of the window is 0."""
        ta, tb, tc = tests
        assert (tb - ta) % 2 == 0, tests
        ref = (sum(base) * threshold) >> 5
        if d23 is None:                           # pa[9] = tests[1] - tests[2] + 3 (pa[2] - pa[3]) must not be negative
            d23 = max(0, -((tb - tc) // 3))
        d1011 = (tb - ta) // 2
        x = ref + tc - 2 * d23 - d1011           # pa[1] + pa[4] + pa[12]
        p9 = ref + ta - x + d23 + d1011
        pa = np.zeros(19, dtype=np.int64)
        pa[5], pa[8], pa[16], pa[17], pa[18] = base
        pa[10], pa[11] = (d1011, 0) if d1011 >= 0 else (0, -d1011)
        pa[2], pa[3] = (d23, 0) if d23 >= 0 else (0, -d23)
        pa[9] = p9
        need = max(0, -min(pre))                  # pa[7], pa[14], pa[15] = pa[1] / pa[12] - margin must stay >= 0
        pa[12] = max(x // 3, need)
        pa[1] = max((x - pa[12]) // 2, need)
        pa[4] = x - pa[12] - pa[1]
        pa[7], pa[14], pa[15] = pa[1] - pre[0], pa[12] - pre[1], pa[12] - pre[2]
        if not ((pa >= 0).all() and (pa <= 65535).all()):
            raise ValueError(f"window not realisable in u16: {pa.tolist()}")
        # self-check of the design against the comparisons themselves
        pv = preamble_verdicts(np.concatenate([pa, np.zeros(1, np.int64)]), threshold)
        assert pv[0][0] == all(m > 0 for m in pre)
        assert [v[0] for v in pv[1:]] == [t >= 0 for t in tests]
        self.mag[j:j + 19] = pa.astype(np.uint16)
        self.windows.append(dict(j=j, pre=tuple(pre), tests=tuple(tests), values=pa))

    def expected(self, threshold):
        """The designed answer: {'frames': the frames expected accepted, in order, 'demod_preambles': n,
        'demod_preamblePhase': [5 counts]} over every scan position of the capture (buffer b scans capture samples
        b * CHUNK - 326 .. + its length; the first buffer's look-behind is 326 zeros), skipping
        msgbits * 12 / 5 positions behind every accepted frame (demod_2400.c:416), up to the end of its buffer."""
        z = np.concatenate([np.zeros(OVERLAP, np.uint16), self.mag, np.zeros(19, np.uint16)])
        npos = self.n                              # positions -326 .. n - 327, i.e. z indices 0 .. n - 1
        parts = [preamble_verdicts(z[k:min(k + (1 << 20), npos) + 19], threshold) for k in range(0, npos, 1 << 20)]
        pre, a, b, c = (np.concatenate([p[i] for p in parts]) if parts else np.zeros(0, bool) for i in range(4))
        live = np.ones(npos, dtype=bool)
        acc = sorted((f for f in self.frames if f["accept"]), key=lambda f: f["j"])
        for f in acc:
            k = f["j"] + OVERLAP                   # the skip ends with the buffer: the next one scans on from its look-behind
            live[k + 1:min(k + 1 + f["msgbits"] * 12 // 5, (k // CHUNK + 1) * CHUNK)] = False
        pa_, pb_, pc_ = (pre & live & a), (pre & live & b), (pre & live & c)
        return {"frames": acc, "demod_preambles": int((pa_ | pb_ | pc_).sum()),
                "demod_preamblePhase": [int(pa_.sum()), int(pa_.sum()), int(pb_.sum()), int(pb_.sum()), int(pc_.sum())]}


def check_frames(msgs, frames, rereads=False):
    """The accepted messages are exactly the designed frames: start position (timestamp), phase and bytes.  rereads:
    a frame read at the last scan positions of a buffer may be read once more from the next buffer's first positions
    (the skip-ahead ends with the buffer), a few ticks later than its design says: such a second reading of the same
    bytes is allowed directly behind it."""
    if rereads:
        keep, prev = [], None
        for m in msgs:
            if prev is not None and bytes(m["msg"]) == bytes(prev["msg"]) and 0 < int(m["timestampMsg"]) - int(prev["timestampMsg"]) < 100:
                continue
            keep.append(m)
            prev = m
        msgs = keep
    assert len(msgs) == len(frames), (len(msgs), [(f["j"], f["phase"], f["df"]) for f in frames])
    for m, f in zip(msgs, frames):
        ts = 5 * (f["j"] + OVERLAP) + (8 + 56) * 12 + f["phase"]   # demod_2400.c:358, j buffer-relative
        assert int(m["bestphase"]) == f["phase"], (int(m["bestphase"]), f["phase"], f["j"])
        assert int(m["timestampMsg"]) == ts, (int(m["timestampMsg"]), ts)
        assert bytes(m["msg"][: f["msgbits"] // 8]) == f["bytes"], (f["j"], f["df"])


def check_counts(stats, exp):
    assert stats["demod_preambles"] == exp["demod_preambles"], (stats["demod_preambles"], exp["demod_preambles"])
    assert list(stats["demod_preamblePhase"]) == exp["demod_preamblePhase"], (stats["demod_preamblePhase"], exp)


def capture_position(b, j):
    """Capture sample of scan position j of buffer b (its look-behind is the 326 samples in front of it)."""
    return b * CHUNK - OVERLAP + j


# ---- the scenes of tests/test_mag_scenes.py and tests/test_gpu_mag_scenes.py ----------------------------------------

FAR = 4


def preamble_cases():
    """(pre margins, test margins): each pre-check comparison one below / equal / one above its bound with the three
    tests passing, and each threshold test one below / equal / one above with the two others failing by FAR."""
    out = []
    for k in range(3):
        for m in (-1, 0, 1):
            pre = [1, 1, 1]
            pre[k] = m
            out.append((tuple(pre), (FAR, FAR, FAR)))
    for m in (-1, 0, 1):
        out.append(((1, 1, 1), (m, m - 2 * FAR, -FAR)))
        out.append(((1, 1, 1), (m - 2 * FAR, m, -FAR)))
        out.append(((1, 1, 1), (-2 * FAR, -2 * FAR, m)))
    return out


EDGES = (0, 1, 2, 15, 16, 17, 31, 32, 2047, 2048, 2049, 4095, 4096, CHUNK // 8 - 1, CHUNK // 8, CHUNK // 4 - 1, CHUNK // 4,
         CHUNK // 2 - 1, CHUNK // 2, CHUNK - 2048, CHUNK - 17, CHUNK - 16, CHUNK - 2)


def preamble_scene(threshold, tail=777):
    """One buffer per case of preamble_cases() (buffer 0 only from position 326 on, behind its zero look-behind): the
    case's window at every position of EDGES, at 16 positions 25 apart (every residue of a 16-position run) and at the
    last scan position CHUNK - 1 (mlen - 1, the last one before the 326-sample overlap); the capture's short last
    buffer (tail samples) has the first case at its mlen - 1.  Two windows whose 19 samples would overlap keep the first.
    The base noise runs through 500 .. 531 from window to window, so that base_noise * threshold >> 5 meets every
    remainder mod 32 an odd threshold can give (the kernel forms ref_level - 1 as (base_noise * threshold - 32) >> 5)."""
    cases = preamble_cases()
    sc = Scene(len(cases) * CHUNK + tail)
    used = np.zeros(sc.n + 64, dtype=bool)

    def put(b, j, case):
        s = capture_position(b, j)
        if s < 0 or s + 19 > sc.n or used[s:s + 20].any():
            return
        used[max(s - 1, 0):s + 20] = True
        base = (100, 100, 100, 100, 100 + len(sc.windows) % 32)
        sc.preamble(s, threshold, pre=case[0], tests=case[1], base=base)

    for b, case in enumerate(cases):
        for j in EDGES + tuple(10000 + 25 * r for r in range(16)) + (CHUNK - 1,):
            put(b, j, case)
    if tail > 19:
        put(len(cases), tail - 1, cases[0])
    return sc


def full_scale_scene():
    """The largest base noise: five samples at 65535 (pa[5], pa[8], pa[16..18]) and the pre-check passing, at every
    residue of a run; ref_level = 327675 * threshold >> 5 (4095937 at 400)."""
    sc = Scene(2 * CHUNK + 1000)
    for r in range(40):
        pa = np.zeros(19, dtype=np.uint16)
        pa[[5, 8, 16, 17, 18]] = 65535
        pa[[1, 4, 9, 12]] = 65535
        pa[[7, 14, 15]] = 65534
        pa[[2, 10]] = 65535
        s = capture_position(1, 20000 + 23 * r)
        sc.mag[s:s + 19] = pa
    return sc


def edge_scene(offsets=None, tail=777):
    """One frame per buffer b, starting at capture sample b * CHUNK + offset for every offset of CHUNK - 400 .. CHUNK + 20
    (the frame read at the last scan positions of a buffer, straddling into its overlap, or at the next buffer's first
    ones), sub-sample ticks, DF17 and DF11 of alternating lengths in turn; and one in the short last buffer read at its
    last scan position."""
    offsets = list(range(CHUNK - 400, CHUNK + 21)) if offsets is None else list(offsets)
    nb = len(offsets) + 1
    sc = Scene(nb * CHUNK + tail, seed=7)
    for b, o in enumerate(offsets):
        sc.frame(b * CHUNK + o, sub=o % 5, df=(17, 11)[b % 2], addr=0x100000 + b, high=(20000, 65535, 3000)[b % 3])
    # short last buffer: read at j = tail - 1 (tick 5 j + 6 - 1 + 2, phase 6)
    j = capture_position(nb, tail - 1)
    sc.frame(j, sub=4, df=11, addr=0xABCDEF)
    return sc


def skip_scene(nbits, fate, seed=0):
    """Skip-ahead (demod_2400.c:416): a first frame (56 or 112 bits) whose own last parity pulses form a passing preamble
    at position j + d, for d = msglen * 12 / 5 - 2 .. + 3, one first frame per d, far apart.  fate: 'accepted' (DF17 /
    DF11 clean), 'bad-crc' (a body bit flipped, nfix 0) or 'unknown' (an AP format of an address never seen).  The
    designed answer counts the preamble at j + d exactly when d > the skip or the first frame was not accepted.

    The preamble at j + d is not a second transmission: a whole frame whose preamble started inside the first frame's
    last bits would overwrite them and break the first frame's CRC.  So the payload of the first frame is drawn until its
    own tail passes the preamble tests at j + d (at SKIP_THRESHOLD the pre-check decides).  What follows each first frame
    is a whole second frame clear of it, its kind cycling with d over DF17, DF11 and an AP format of the first frame's
    address (known only when the first one was accepted): it shows where the scan resumes and what the first frame's fate
    left in the filter, not the skip boundary itself."""
    rng = np.random.default_rng(seed)
    skip = nbits * 12 // 5
    sc = Scene(4 * CHUNK + 100, seed=seed)   # five buffers: a batch the GPU resolve takes
    df1 = {"accepted": 17 if nbits == 112 else 11, "bad-crc": 17 if nbits == 112 else 11,
           "unknown": 20 if nbits == 112 else 4}[fate]
    pos = 2000
    for d in range(skip - 2, skip + 4):
        for _ in range(5000):                   # a payload whose tail passes the preamble tests at j + d
            addr = int(rng.integers(1, 1 << 24))  # (a DF11 body is DF, CA and address: new address, new parity)
            bits = frame_bits(rng, df1, addr, flip=(20,) if fate == "bad-crc" else ())
            sub = int(rng.integers(0, 5))
            trial = Scene(1200)
            f = trial.frame(300, sub=sub, bits=bits)
            v = preamble_verdicts(trial.mag[f["j"] + d:f["j"] + d + 20].astype(np.int64), SKIP_THRESHOLD)
            if v[0][0] and (v[1][0] or v[2][0] or v[3][0]):
                break
        else:
            raise AssertionError("no payload found")
        f = sc.frame(pos, sub=sub, bits=bits, accept=fate == "accepted")
        f["d"] = d
        end = pos + 40 + nbits * 12 // 5
        kind = (17, 11, "ap")[(d - skip + 2) % 3]
        df2 = {17: 17, 11: 11, "ap": 20 if nbits == 112 else 4}[kind]
        a2 = addr if kind == "ap" else int(rng.integers(1, 1 << 24))
        sc.frame(end + 30, sub=d % 5, df=df2, addr=a2, accept=(kind != "ap") or fate == "accepted")
        pos += 1500
    return sc


SKIP_THRESHOLD = 1   # the skip scenes run at --preamble-threshold 1: the pre-check decides

TIE_FIXES = ((0, ()), (1, (40,)), (2, (40,)), (2, (40, 77)))


def tie_scene(nfix, flips, seed=3):
    """Phase ties: DF17 frames (clean, or with flipped bits that --fix / --aggressive correct) at every sub-sample tick,
    each read alike from T - 2 .. T, so two or three trial phases score the same: the lowest-numbered phase of the first
    position must win (demod_2400.c strict `>`), and demod_bestPhase counts it."""
    sc = Scene(4 * CHUNK + 100, seed=seed)
    for k in range(40):
        sc.frame(3000 + 700 * k, sub=k % 5, df=17, addr=0x3C0000 + k, flip=flips, high=(20000, 65535, 1200, 30000)[k % 4])
    return sc


def filter_scene(seed=5):
    """ICAO filter order (mode_s.c:717-726) inside one batch of 6 buffers: every case is at position ~1000 + 3000 k of
    its buffer."""
    sc = Scene(6 * CHUNK + 500, seed=seed)
    A, B, Cc, D, E, F = 0xA1A1A1, 0xB2B2B2, 0xC3C3C3, 0xD4D4D4, 0xE5E5E5, 0xF6F6F6
    s = capture_position
    # buffer 0: AP of A before the DF11 that adds A, then AP of A after it; DF11 with IID 3 of B (unknown: rejected)
    sc.frame(s(0, 1000), 2, df=4, addr=A, accept=False)
    sc.frame(s(0, 4000), 1, df=11, addr=A)
    sc.frame(s(0, 7000), 3, df=20, addr=A)
    sc.frame(s(0, 10000), 0, df=11, addr=B, parity_xor=3, accept=False)
    # buffer 1: AP of A (known from buffer 0); corrected DF17 of unknown C (nfix >= 1), then AP of C: still unknown;
    # corrected DF11 (IID 0) of known A: accepted, adds nothing; corrected DF11 of unknown F: rejected (mode_s.c:449-465)
    sc.frame(s(1, 1000), 4, df=5, addr=A)
    sc.frame(s(1, 4000), 2, df=17, addr=Cc, flip=(50,))
    sc.frame(s(1, 7000), 2, df=21, addr=Cc, accept=False)
    sc.frame(s(1, 10000), 1, df=11, addr=A, flip=(21,))   # an address bit: the syndrome leaves IID 0
    sc.frame(s(1, 13000), 3, df=11, addr=F, flip=(40,), accept=False)
    sc.frame(s(1, 16000), 0, df=20, addr=F, accept=False)
    # buffer 2: D's first clean squitter inside the skip of the DF17 in front of it, never read, so D is never added;
    # then corrected DF17s of D (unknown: lower score) and an AP of D (rejected).  For the GPU resolver's probation table
    # (msd_resolve_kernels.hip) this is the path of an entry that fails its probation: D's later tries were staged as
    # known behind a message that is not accepted, and must go back to unknown.  It is not the interleaving the
    # aa70d10 fix is about (a confirmation taken back because the cut moved in front of the confirming message):
    # that one needs overlapping transmissions of two new aircraft, which a scene of separate frames does not build.
    x = sc.frame(s(2, 1000), 1, df=17, addr=E, high=30000)
    sc.frame(x["sample"] + 200, 3, df=17, addr=D, high=3000, accept=False)
    sc.frame(s(2, 6000), 0, df=17, addr=D, flip=(33,))
    sc.frame(s(2, 9000), 4, df=0, addr=D, accept=False)
    sc.frame(s(2, 12000), 2, df=17, addr=D, flip=(90,))
    # buffers 3-5: the AP of A in each (known unless the filter forgot it: see the flip test) and a DF11 of B (adds B)
    for b in (3, 4, 5):
        sc.frame(s(b, 1000), b % 5, df=16 if b % 2 else 4, addr=A)
    sc.frame(s(3, 4000), 1, df=11, addr=B)
    sc.frame(s(4, 4000), 1, df=20, addr=B)
    return sc


def flip_scene(C=CHUNK):
    """A filter flip inside a batch (icao_filter.c:145-160, every 60 s of the clock): three batches of four buffers; the
    DF11 that adds A in buffer 1, an AP format of A in every buffer (those of buffers 0 and 1 come before the DF11: rejected).  The
    live feed drops D1 samples in front of batch 2 -- its first buffer starts at 60.0004 s: the flip after it keeps A in
    the older half -- and D2 in front of batch 3, whose buffer 1 starts at 120 s: the flip after buffer 1 forgets A, so
    the AP formats of buffers 2 and 3 are rejected.  Returns (scene, drops)."""
    sc = Scene(12 * C, seed=11)
    A = 0x5A5A5A
    for b in range(12):
        sc.frame(b * C + 1000, b % 5, df=(4, 20, 5, 21, 0, 16)[b % 6], addr=A, accept=2 <= b < 10)
        if b == 1:
            sc.frame(b * C + 5000, 2, df=11, addr=A)
    sc.frames.sort(key=lambda f: f["j"])
    d1 = 144000000 + 1000 - 4 * C
    d2 = 288000000 - C - 8 * C - d1
    return sc, [0, d1, d2]
