"""Constructed u16 magnitude captures for the Mode A/C demodulator, with a designed answer: plain numpy, no product or
oracle code.  The companion of mag_scenes.py (whose Scene, CHUNK, OVERLAP and capture_position it reuses) for
demodulate2400AC (demod_2400.c:522-708).

Every decision of that function is an exact comparison of integers (the pulse test :581-592, the bit windows :641-668)
or of a float32 rounded once (the clock :597-600, the thresholds :623-625), and generated traffic reaches their bounds
only by chance.  A scene places every pulse at an exact sample and an exact level of a chosen buffer instead.  All
positions are those of the scanning buffer's own array, look-behind first: position j of buffer b is capture sample
b * CHUNK - 326 + j, and the loop scans 1 <= j < mlen, so the last 326 samples of a buffer (and of the capture) are
scanned by the next buffer only (or never).

The module has its own restatement of the per-buffer noise level (convert.c:104-110, demod_2400.c:530-531), the pulse
test, the clock, the two thresholds, the twenty windows and the 13-bit mapping.  AcScene.reply() renders a reply whose
F1 is scanned at (buffer, position), says how it is designed to end (DELIVERED, or the stage that rejects it) and
returns the designed (timestampMsg, modeac).  finish() then asserts the design on the finished capture: every buffer
whose noise level a reply was designed against has exactly that level (settle() iterates a scene to that fixed point), every
designed reply ends at its designed stage, and a scan of the whole capture by the restatement delivers the designed
replies and nothing else.  expected() is that designed list.  Scenes that are dense on purpose (dense_scene) have no
reply-by-reply design: their expected() is the restatement's scan, and they assert the figures they were built for.
"""
import functools
import math

import numpy as np

from mag_scenes import CHUNK, OVERLAP, Scene, capture_position

F32 = np.float32
SKIP = 20 * 87 // 25                         # demod_2400.c:705
TILE = 1024                                  # F1 positions of one wavefront tile of the candidate kernel
SEGMENT = 1280                               # candidates of a buffer the GPU resolver stages at a time
F1, F2, X1, SPI = 0, 14, 7, 17               # window numbers
GUESS = 1000                                 # the noise level a scene is designed against before settle() has measured it
QUIET = (7, 15, 16, 18, 19)
# window number -> bit of the delivered code (demod_2400.c:672-685)
CODE_BITS = {1: 0x0010, 2: 0x1000, 3: 0x0020, 4: 0x2000, 5: 0x0040, 6: 0x4000, 8: 0x0100, 9: 0x0001, 10: 0x0200,
             11: 0x0002, 12: 0x0400, 13: 0x0004, 17: 0x0080}
DELIVERED, HIDDEN, UNSCANNED = "delivered", "hidden", "unscanned"   # ... or a stage of read(): f1, f2, framing, quiet, noisy, uncertain


def code_of(index):
    """The index-th of the 4096 codes: four octal digits A B C D as the delivered value holds them."""
    return ((index >> 9) & 7) << 12 | ((index >> 6) & 7) << 8 | ((index >> 3) & 7) << 4 | (index & 7)


def noise_level_of(own):
    """demod_2400.c:530-531 on the integer sums of convert.c:104-110 over a buffer's own samples (None: empty buffer)."""
    n = int(own.size)
    if n == 0:
        return None
    v = own.astype(np.uint64)
    mean_level = int(v.sum()) / 65536.0 / n
    mean_power = int((v * v).sum()) / 65535.0 / 65535.0 / n
    return int((mean_power + math.sqrt(mean_power - mean_level * mean_level)) * 65535 + 0.5)


def pulse_level(x, s, noise):
    """The pulse test (:581-592, :608-619) at sample s: the level, or None."""
    if not x[s - 1] < x[s]:
        return None
    if x[s + 2] > x[s] or x[s + 2] > x[s + 1]:
        return None
    level = (x[s] + x[s + 1]) // 2
    if noise * 2 > level:
        return None
    return level


def clock_of(pos, m0, m1):
    """f1_clock (:597-600), every operation in float32 and rounded once, the last addition in double."""
    a, b = F32(m0) * F32(m0), F32(m1) * F32(m1)
    fraction = b / (a + b)
    return int(float(F32(25) * (F32(pos) + fraction * fraction)) + 0.5)


def thresholds_of(noise, level):
    """(signal_threshold, noise_threshold), :623-625: float32 sqrt of the u32 product, double multiply and divide."""
    mid = float(np.sqrt(F32((noise * level) & 0xFFFFFFFF), dtype=F32))
    return int(mid * math.sqrt(2.0) + 0.5), int(mid / math.sqrt(2.0) + 0.5)


def read(x, pos, noise):
    """One F1 position of a buffer's array x (ints): (stage, f2_clock, code); stage 'ok' or the first test that rejects."""
    l1 = pulse_level(x, pos, noise)
    if l1 is None:
        return "f1", None, None
    clock = clock_of(pos, x[pos], x[pos + 1])
    f2_clock = clock + 87 * 14
    l2 = pulse_level(x, f2_clock // 25, noise)
    if l2 is None:
        return "f2", f2_clock, None
    sig, quiet = thresholds_of(noise, max(l1, l2))
    on, noisy, uncertain = set(), False, False
    for k in range(20):
        s = (clock + 87 * k) // 25
        if x[s + 2] >= sig:
            noisy = True
        if x[s] >= sig or x[s + 1] >= sig:
            on.add(k)
        elif x[s] > quiet and x[s + 1] > quiet:
            uncertain = True
    if F1 not in on or F2 not in on:
        return "framing", f2_clock, None
    if on & set(QUIET):
        return "quiet", f2_clock, None
    if noisy:
        return "noisy", f2_clock, None
    if uncertain:
        return "uncertain", f2_clock, None
    return "ok", f2_clock, sum(CODE_BITS[k] for k in on if k in CODE_BITS)


class AcScene(Scene):
    """A capture of n u16 magnitudes with Mode A/C replies (and, through Scene.frame, Mode S frames)."""

    def __init__(self, n, levels=None, seed=0):
        super().__init__(n, 0, seed)
        self.assumed = dict(levels or {})     # buffer -> the noise level its replies are designed against
        self.used = set()                     # the buffers whose assumed level a design depends on
        self.replies = []
        self.designed = True

    @property
    def nbuffers(self):
        return self.n // CHUNK + 1            # a capture that ends on a buffer boundary ends with an empty buffer

    def mlen(self, b):
        return max(0, min(CHUNK, self.n - b * CHUNK))

    def level(self, b):
        """The noise level buffer b is designed against (GUESS until settle() has measured it)."""
        self.used.add(b)
        return self.assumed.get(b, GUESS)

    def noise_levels(self):
        return [noise_level_of(self.mag[b * CHUNK:(b + 1) * CHUNK]) for b in range(self.nbuffers)]

    def put(self, b, j, values):
        s = capture_position(b, j)
        values = np.asarray(values, dtype=np.int64)
        assert s >= 0 and s + values.size <= self.n and values.min() >= 0 and values.max() <= 65535, (b, j, values)
        self.mag[s:s + values.size] = values

    def array(self, b):
        """Buffer b's array as the demodulator sees it: 326 samples of look-behind, its own, zeros behind."""
        lo = b * CHUNK - OVERLAP
        x = np.zeros(OVERLAP + self.mlen(b) + 80, dtype=np.int64)
        a, e = max(lo, 0), min(lo + OVERLAP + self.mlen(b) + 80, self.n)
        x[a - lo:e - lo] = self.mag[a:e]
        return x

    def reply(self, b, pos, code=0, spi=False, level=60000, f1=None, f2=None, expect=DELIVERED, missing=(), extra=(),
              windows=None, render=True):
        """A reply whose F1 is scanned at position pos of buffer b.  f1 / f2: the four samples (s - 1 .. s + 2) of that
        framing pulse instead of the flat (0, level, level, 0); every other pulse is the flat pair (level, level) at its
        window's two samples, found from the clock of F1.  missing / extra: windows left out / added; windows: {k: (x0,
        x1, x2)} written as they are.  render=False: nothing is written -- a second position that reads a reply already
        there.  Returns the designed record: ts, code, expect."""
        m = f1 if f1 is not None else (0, level, level, 0)
        clock = clock_of(pos, m[1], m[2]) if m[1] or m[2] else 25 * pos
        code = code | (0x0080 if spi else 0)
        on = {k for k, bit in CODE_BITS.items() if code & bit} | {F2} | set(extra)
        r = dict(b=b, pos=pos, clock=clock, code=code, expect=expect, ts=b * CHUNK * 5 + (clock + 87 * 14) // 5)
        self.replies.append(r)
        if not render:
            return r
        for k in sorted(on - set(missing) - {F1}):
            self.put(b, (clock + 87 * k) // 25, (level, level))
        if f2 is not None:
            self.put(b, (clock + 87 * F2) // 25 - 1, f2)
        for k, v in (windows or {}).items():
            self.put(b, (clock + 87 * k) // 25, v)
        if f1 is not None:
            self.put(b, pos - 1, m)
        elif F1 not in missing:
            self.put(b, pos, m[1:3])
        return r

    def reply_at(self, sample, **kw):
        """reply() by capture sample: in the buffer that scans it."""
        b = (sample + OVERLAP) // CHUNK
        return self.reply(b, sample + OVERLAP - b * CHUNK, **kw)

    def scan(self):
        """The restatement over the whole capture: [(timestampMsg, code, buffer, position)] with the skip-ahead."""
        out = []
        for b, noise in enumerate(self.noise_levels()):
            mlen = self.mlen(b)
            if mlen < 2:
                continue
            x = self.array(b)
            j = np.arange(1, mlen)
            cand = j[(x[j - 1] < x[j]) & (x[j + 2] <= x[j]) & (x[j + 2] <= x[j + 1]) & (2 * noise <= (x[j] + x[j + 1]) // 2)]
            xl, resume = x.tolist(), 0
            for p in cand.tolist():
                if p < resume:
                    continue
                stage, f2_clock, code = read(xl, p, noise)
                if stage == "ok":
                    out.append((b * CHUNK * 5 + f2_clock // 5, code, b, p))
                    resume = p + SKIP + 1
        return out

    def finish(self):
        """Assert the design on the finished capture (module doc) and return the scene."""
        levels = self.noise_levels()
        for b in sorted(self.used):
            assert levels[b] == self.assumed.get(b, GUESS), ("designed against another level", b, levels[b], self.assumed.get(b))
        self.scanned = self.scan()
        self.answer = [(t, c) for t, c, _, _ in self.scanned]
        if not self.designed:
            return self
        arrays = {}
        delivered = {(b, p) for _, _, b, p in self.scanned}
        for r in self.replies:
            b, pos = r["b"], r["pos"]
            if not 1 <= pos < self.mlen(b):
                assert r["expect"] == UNSCANNED, r
                continue
            if b not in arrays:
                arrays[b] = self.array(b).tolist()
            stage, f2_clock, code = read(arrays[b], pos, levels[b])
            if r["expect"] in (DELIVERED, HIDDEN):
                assert (stage, code) == ("ok", r["code"]) and b * CHUNK * 5 + f2_clock // 5 == r["ts"], (r, stage, code)
                assert ((b, pos) in delivered) == (r["expect"] == DELIVERED), r
            else:
                assert stage == r["expect"], (r, stage)
        want = [(r["ts"], r["code"]) for r in sorted(self.replies, key=lambda r: (r["b"], r["pos"])) if r["expect"] == DELIVERED]
        extra = sorted(set((t, c, b, p) for t, c, b, p in self.scanned) - {(r["ts"], r["code"], r["b"], r["pos"]) for r in self.replies})
        assert self.answer == want, ("the capture holds a reply that was not designed", extra[:5])
        self.answer = want
        return self

    def expected(self):
        """{'replies': [(timestampMsg, code)] in delivery order, 'demod_modeac': n} -- the designed answer."""
        return {"replies": list(self.answer), "demod_modeac": len(self.answer)}

    def count(self, *expect):
        return sum(r["expect"] in expect for r in self.replies)


def fill(sc):
    """A plain reply in every buffer that has nothing of its own: a silent buffer has noise level 0 and rejects all."""
    for b in range(sc.nbuffers):
        if sc.mlen(b) > 1200 and not sc.mag[b * CHUNK:(b + 1) * CHUNK].any():
            sc.reply(b, 1000, code=0x0300 + b)["fill"] = True
    return sc


def settle(build):
    """build(levels) -> AcScene designed against the per-buffer noise levels `levels`; rebuilt until the levels it was
    designed against are the ones its capture has (a pulse a unit above or below a bound barely moves the sums)."""
    levels = {}
    for _ in range(10):
        sc = build(levels)
        actual = sc.noise_levels()
        if all(actual[b] == levels.get(b, GUESS) for b in sc.used):
            return sc.finish()
        levels = {b: v for b, v in enumerate(actual) if v is not None}
    raise AssertionError("the noise levels do not settle")


def check_replies(msgs, exp):
    """The delivered Mode A/C records (msgtype 32) are the designed replies: timestamp and code, in order."""
    ac = msgs[msgs["msgtype"] == 32]
    got = [(int(m["timestampMsg"]), (int(m["msg"][0]) << 8) | int(m["msg"][1])) for m in ac]
    assert len(got) == len(exp["replies"]), (len(got), len(exp["replies"]))
    assert got == exp["replies"], next((i, g, w) for i, (g, w) in enumerate(zip(got, exp["replies"])) if g != w)


# ---- the scenes of tests/test_ac_scenes.py and tests/test_gpu_ac_scenes.py -------------------------------------------

def pulse_cases(noise):
    """(five samples s - 1 .. s + 3 of a framing pulse, passes the pulse test, level of the other framing pulse) at every
    comparison's bound; the level bound against the buffer's noise level `noise`.  A case that passes leaves the reply
    decodable: its larger sample is above the signal threshold and its third below it.  Where the second sample is the
    larger one, the fourth is one above the third, so that the next position (whose pulse would be samples two and
    three, with the same clock) fails: the case alone decides whether the reply is delivered.  None: passes the pulse
    test, and its third sample then spoils window 0."""
    hi, low = 60000, 2 * noise + 400
    out = []
    for m0 in (1, 2000):                              # m[s - 1] vs m[s]
        for d in (-1, 0, 1):
            out.append(((m0 + d, m0, hi, 0, 1), d < 0, hi))
    for m0 in (60000, 65535):
        for d in (-1, 0, 1):
            if m0 + d <= 65535:
                out.append(((m0 + d, m0, m0, 0, 0), d < 0, hi))
    for m0 in (1, 700):                               # m[s + 2] vs m[s], the smaller of the two
        for d in (-1, 0, 1):
            out.append(((0, m0, hi, m0 + d, m0 + d + 1), d <= 0, hi))
    for m1 in (0, 1, 700):                            # m[s + 2] vs m[s + 1], the smaller of the two
        for d in (-1, 0, 1):
            if m1 + d >= 0:
                out.append(((0, hi, m1, m1 + d, 0), d <= 0, hi))
    for d in (-2, -1, 0, 1):                          # m0 + m1 vs 4 noise: 4 noise + 1 is odd, and / 2 floors it onto the bound
        out.append(((0, noise, 3 * noise + d, 0, 1), d >= 0, low))
        out.append(((0, 3 * noise + d, noise, 0, 0), d >= 0, low))
    out.append(((0, 65535, 65535, 65535, 0), None, hi))
    return out


def pulse_scene(which):
    """Scene a.  which='f1': every case of pulse_cases() as the F1 pulse, at every residue mod 16 of the position, in
    lane 0 (positions 0..15) and lane 63 (1008..1023) of a tile, one reply per tile.  which='f2': every case as the F2
    pulse, once, behind an F1 of (58000, 60000), whose clock keeps window 13 clear of the sample in front of F2.  The
    data pulses are at 60000, C1 is off."""
    ncase = len(pulse_cases(GUESS))
    tiles = ncase * 32 if which == "f1" else ncase
    nb = max((tiles + 1) // (CHUNK // TILE) + 1, 4)                      # (a batch of four buffers: the GPU resolve stage takes it)

    def build(levels):
        sc = AcScene(nb * CHUNK + 500, levels, seed=1)
        t = 1
        for rep in range(32 if which == "f1" else 1):
            for i in range(ncase):
                b, tile = t // (CHUNK // TILE), t % (CHUNK // TILE)
                t += 1
                shape, ok, other = pulse_cases(sc.level(b))[i]
                code = code_of(7 * i + rep) & ~0x0010
                if which == "f1":
                    pos = tile * TILE + (rep if rep < 16 else 1008 + rep - 16)
                    expect = DELIVERED if ok else ("noisy" if ok is None else "f1")
                    sc.reply(b, pos, code=code, expect=expect, f1=shape[:4], f2=(0, other, other, 0))
                    sc.put(b, pos + 3, shape[4:])
                else:
                    expect = DELIVERED if ok else ("noisy" if ok is None else "f2")
                    lead = (0, 58000, 60000, 0) if other == 60000 else (0, other - 300, other, 0)
                    sc.reply(b, tile * TILE + 300 + i, code=code, expect=expect, f1=lead, f2=shape[:4])
        return fill(sc)

    return settle(build)


def edge_scene(tail=3000):
    """Scene b: F1 at the first and last position of a tile (the last one has its F2 and its windows in the 72 samples
    staged beyond the tile), at positions 1 and 0 of a buffer (the loop starts at 1), at mlen - 1 of a full buffer and of
    the ragged last one, in the last buffer's look-behind and in its unscanned tail, and with m1 >> m0 (the clock a whole
    sample late: the farthest reach of window 19) at a tile's and at a buffer's last position."""
    sc = AcScene(4 * CHUNK + tail, seed=2)
    late = (0, 300, 60000, 0)
    for b in range(4):
        for tile, p in ((1, 0), (2, 1023), (5, 1022), (7, 1), (127, 0), (127, 700)):
            sc.reply(b, tile * TILE + p, code=code_of(64 * b + tile + p))
        sc.reply(b, 9 * TILE + 1023, code=0x7777, spi=True, f1=late)
        sc.reply(b, 11 * TILE + 1023 - 69, code=0x1234)                  # its skip ends with the tile
    sc.reply(1, 1, code=0x0101)
    sc.reply(1, CHUNK - 1, code=0x4321, f1=late)
    sc.reply(3, 0, code=0x0202, expect=UNSCANNED)                       # = position CHUNK of buffer 2
    sc.reply(4, 150, code=0x0505)                                        # in the ragged buffer's look-behind
    sc.reply(4, tail - 1, code=0x0606, spi=True, f1=late)
    sc.reply(4, tail - 200, code=0x0707)
    sc.reply(4, tail + 100, code=0x0303, expect=UNSCANNED)
    return sc.finish()


def clock_pairs(pos, side):
    """Float32 search: (m0, m1) whose 25 * (pos + fraction^2) lies within two ulps of some k + 0.5, below it (side -1) or
    at / above it (+1); first choice a pair whose clock changes when fraction^2 is added to the position in one
    contracted multiply-add."""
    m1 = np.arange(3000, 65536, dtype=np.int64)
    fallback = None
    for m0 in range(30000, 65536, 1871):
        a, b = F32(m0) * F32(m0), m1.astype(F32) * m1.astype(F32)
        fr = b / (a + b)
        clk = (F32(25) * (F32(pos) + fr * fr)).astype(np.float64)
        fused = (F32(25) * (np.float64(pos) + fr.astype(np.float64) * fr.astype(np.float64)).astype(F32)).astype(np.float64)
        d = clk - (np.floor(clk) + 0.5)
        near = (np.abs(d) <= 2 * np.spacing(clk.astype(F32)).astype(np.float64)) & ((d < 0) if side < 0 else (d >= 0))
        best = np.flatnonzero(near & (np.floor(clk + 0.5) != np.floor(fused + 0.5)))
        if best.size:
            return m0, int(m1[best[0]]), True
        if fallback is None and near.any():
            fallback = (m0, int(m1[np.flatnonzero(near)[0]]), False)
    assert fallback is not None, pos
    return fallback


def clock_scene():
    """Scene c: F1 pairs (m0, m1) that put f1_clock on each of 25 f1 + 0 .. 25, and pairs within two float32 ulps of a
    half on either side (clock_pairs), at small positions and at positions above 65536, where float32 holds fewer
    fraction bits.  All are delivered; the timestamp (f2_clock / 5) is the check."""
    sc = AcScene(4 * CHUNK + 2000, seed=3)
    sc.clocks, sc.contracted = set(), 0
    for base in (700, 66000):
        for c in range(26):
            fr = math.sqrt(min(max(c, 0.3), 24.8) / 25.0)                # fraction^2 = c / 25, inside its interval
            m0, m1 = (60000, round(60000 * math.sqrt(fr / (1 - fr)))) if fr < 0.5 else (round(60000 * math.sqrt((1 - fr) / fr)), 60000)
            pos = base + 150 * c
            r = sc.reply(0, pos, code=code_of(100 + c), f1=(0, m0, m1, 0))
            assert r["clock"] - 25 * pos == c, (c, m0, m1, r["clock"] - 25 * pos)
            sc.clocks.add((base, c))
        for i in range(16):
            pos = base + 150 * 26 + 157 * i
            m0, m1, differs = clock_pairs(pos, -1 if i % 2 else 1)
            sc.contracted += differs
            sc.reply(0, pos, code=code_of(200 + i), f1=(0, m0, m1, 0))
    return fill(sc).finish()


def window_scene():
    """Scene d: one window of a reply (window 5, C4; F1 and F2 flat at 60000) with x0, x1, x2 each one below, at and one
    above the signal threshold; x0 and x1 at the noise threshold and one above, together (uncertain) and one alone
    (off); each framing pulse present but below the signal threshold; each quiet window and X1 holding a pulse."""
    K = 5

    def build(levels):
        sc = AcScene(4 * CHUNK + 2000, levels, seed=4)
        noise = sc.level(0)
        sig, quiet = thresholds_of(noise, 60000)
        pos = iter(range(1000, CHUNK, 300))
        base = 0x4302                                                     # A4 B1 B2 D2: no two pulses 14 windows apart
        for d in (-1, 0, 1):
            on = CODE_BITS[K] if d >= 0 else 0
            sc.reply(0, next(pos), code=base | on, windows={K: (sig + d, 0, 0)})
            sc.reply(0, next(pos), code=base | on, windows={K: (0, sig + d, 0)})
            sc.reply(0, next(pos), code=base | on, windows={K: (quiet, sig + d, 0)})
            sc.reply(0, next(pos), code=base | CODE_BITS[K], windows={K: (60000, 60000, sig + d)},
                     expect=DELIVERED if d < 0 else "noisy")
            sc.reply(0, next(pos), code=base, windows={K: (0, 0, sig + d)}, expect=DELIVERED if d < 0 else "noisy")
        for x0, x1 in ((0, 0), (1, 0), (0, 1), (1, 1)):
            sc.reply(0, next(pos), code=base, windows={K: (quiet + x0, quiet + x1, 0)},
                     expect="uncertain" if x0 and x1 else DELIVERED)
        sc.reply(0, next(pos), code=base, windows={K: (sig - 1, sig - 1, sig - 1)}, expect="uncertain")
        low = 2 * noise + 10                                              # passes the pulse test, reads as no pulse
        sc.reply(0, next(pos), code=base, f1=(0, low, low, 0), expect="framing")
        sc.reply(0, next(pos), code=base, f2=(0, low, low, 0), expect="framing")
        for k in QUIET:
            sc.reply(0, next(pos), code=base, extra=(k,), expect="quiet")
            sc.reply(0, next(pos), code=base, spi=True, windows={k: (0, sig, 0)}, expect="quiet")
            sc.reply(0, next(pos), code=base, spi=True, windows={k: (sig - 1, 0, 0)})
        return fill(sc)

    return settle(build)


def codes_scene(spacing=280, level=60000):
    """Scene e: all 4096 codes without and with SPI, one reply every `spacing` samples, the codes in a scattered order
    so that every buffer holds a like mix; every buffer's 2 * noise_level stays at or below the pulse level."""
    order = (np.arange(8192) * 3001) % 8192
    sc = AcScene(400 + 8192 * spacing + 1000, seed=5)
    for i, v in enumerate(order.tolist()):
        s = 400 + i * spacing
        if (s + OVERLAP) % CHUNK == 0:
            s += 1
        sc.reply_at(s, code=code_of(v & 4095), spi=v >= 4096, level=level)
    sc.finish()
    assert all(2 * v <= level for v in sc.noise_levels() if v is not None)
    assert len(set(sc.expected()["replies"])) == 8192 and {c for _, c in sc.expected()["replies"]} == \
        {code_of(i) | s for i in range(4096) for s in (0, 0x80)}
    return sc


def skip_scene():
    """Scene f: a second reply d = 68 .. 71 samples behind a first (68: its F1 spoils the first one's last window and it is
    delivered itself; 69: hidden by the skip; 70, 71: both delivered), inside a tile and across a tile boundary; the
    d = 69 pair with the first reply spoiled by a pulse in X1 (the second is delivered); the d = 69 pair split by a
    buffer boundary (the skip does not carry: both delivered); pulses with shoulders (a, A, b): b <= a makes two adjacent
    positions pass everything with the same code and clock, the earlier is delivered and hides the later, and a reply 70
    behind it is delivered; b = a + 1 fails the earlier position, and the reply is hidden by the later one's skip."""
    sc = AcScene(4 * CHUNK + 4000, seed=6)                                # five buffers: a batch the GPU resolve stage takes
    for i, d in enumerate((68, 69, 70, 71)):
        for p in (3 * TILE + 100 + 700 * i, (9 + i) * TILE + 994):       # the second one in the same tile / in the next
            sc.reply(0, p, code=0x1010 + d, expect="noisy" if d == 68 else DELIVERED)
            sc.reply(0, p + d, code=0x2020 + d, expect=HIDDEN if d == 69 else DELIVERED)
    sc.reply(0, 20000, code=0, extra=(X1,), expect="quiet")
    sc.reply(0, 20069, code=0x0040)
    sc.reply(0, CHUNK - 10, code=0)                                       # (a code whose pulses buffer 1 cannot read as a reply)
    sc.reply(1, 59, code=0x0444)                                          # position CHUNK + 59 of buffer 0
    cases = ((2000, 2000, 0), (2000, 1999, 0), (2000, 2001, 0), (2000, 0, 1), (2000, 2001, 1), (1, 1, 0), (1, 2, 0), (1, 0, 1))
    for i, (a, b2, tile_edge) in enumerate(cases):
        p = (5 + 2 * i) * TILE + (1023 if tile_edge else 11)                  # tile_edge: the two positions in two tiles
        early = b2 <= a
        sc.reply(1, p, code=0x0555, f1=(0, a, 60000, b2), expect=DELIVERED if early else "f1")
        sc.reply(1, p + 1, code=0x0555, f1=(a, 60000, b2, 0), expect=HIDDEN if early else DELIVERED, render=False)
        sc.reply(1, p + 70, code=0x0666, expect=DELIVERED if early else HIDDEN)
    return fill(sc).finish()


def filler_for(target, base):
    """A block (k samples at 65535 and one more) that brings the buffer `base` (u16, zeros where the block goes: its last
    8000 samples) to the noise level `target`, by bisection on the block's sum of squares."""
    def with_block(k, v):
        own = base.copy()
        own[own.size - 8000:own.size - 8000 + k] = 65535
        own[own.size - 8000 + k] = v
        return own
    lo, hi = 0, 7990 * 65536                                             # k * 65536 + v
    while lo < hi:
        mid = (lo + hi) // 2
        if noise_level_of(with_block(mid >> 16, mid & 65535)) < target:
            lo = mid + 1
        else:
            hi = mid
    own = with_block(lo >> 16, lo & 65535)
    return own, noise_level_of(own)


def dense_scene():
    """Scene g.  Buffer 0: a reply (F1, C2, SPI, F2 at 60000) every 70 samples over the whole buffer: noise_level above
    0x4000 (the candidate kernel's unpacked F1 test) and more than 1280 accepted replies (a second staging segment of
    the GPU resolver); twenty replies in the middle are 69 apart, so that every other one is hidden and the skip-ahead of
    the first segment's last reply hides the second segment's first candidate.  Buffers 1 and 2: replies 400 apart, one with F1 exactly at the level bound and one a unit below it, and
    a filler block tuned to noise levels 0x3fff (the packed test's largest) and 0x4000 (the unpacked test's smallest).
    Buffer 3: a normal buffer with 600 periods of (58000, 60000, 0, 0, 0, 0, 0): two positions in seven pass the F1 test
    and, 49 and 48 samples on, the F2 test (294 in a tile: five rounds of 64), and all fail the windows.  Buffer 4:
    silent (noise_level 0: both thresholds 0, every window reads as a noisy pulse) with a reply in its look-behind;
    buffer 5 has content again.  Not designed reply by reply: expected() is the restatement's scan."""
    sc = AcScene(5 * CHUNK + 3000, seed=7)
    sc.designed = False
    p, k = OVERLAP + 10, 0
    while p < CHUNK + OVERLAP - 80:                                       # 70 apart; 69 behind the candidates 1271 .. 1290
        sc.reply(0, p, code=0x0020, spi=True)
        p += 69 if 1271 <= k <= 1290 else 70
        k += 1
    for b, target in ((1, 0x3fff), (2, 0x4000)):
        for p in range(1000, CHUNK - 9000, 400):
            sc.reply(b, p, code=code_of(p // 400 + b))
        flat = (0, 2 * target + 400, 2 * target + 400, 0)                 # F1 at the level bound 4 noise_level, and a unit below
        sc.reply(b, 400, code=0x0700, f1=(0, target, 3 * target, 0), f2=flat)
        sc.reply(b, 700, code=0x0007, f1=(0, target, 3 * target - 1, 0), f2=flat, expect="f1")
        own, got = filler_for(target, sc.mag[b * CHUNK:(b + 1) * CHUNK])
        sc.mag[b * CHUNK:(b + 1) * CHUNK] = own
        assert got == target, (got, target)
    for p in range(1000, 60000, 500):
        sc.reply(3, p, code=code_of(p // 500))
    sc.train = (3, 70000, 600)
    sc.put(3, 70000, np.tile([58000, 60000, 0, 0, 0, 0, 0], 600))
    sc.reply(4, 100, code=0x0123, expect="quiet")
    sc.reply(5, 700, code=0x0321)
    sc.finish()
    levels = sc.noise_levels()
    per_buffer = [sum(1 for _, _, b, _ in sc.scanned if b == k) for k in range(6)]
    assert levels[0] >= 0x4000 and per_buffer[0] > 1280, (levels, per_buffer)
    # the GPU resolver stages a buffer's candidates (the positions that pass every test) 1280 at a time: the last of the
    # first segment is delivered, the first of the second is 69 behind it and hidden, the next is delivered
    x0 = sc.array(0)
    j = np.arange(1, CHUNK)
    f1 = j[(x0[j - 1] < x0[j]) & (x0[j + 2] <= x0[j]) & (x0[j + 2] <= x0[j + 1]) & (2 * levels[0] <= (x0[j] + x0[j + 1]) // 2)]
    xl = x0.tolist()
    cands = [q for q in f1.tolist() if read(xl, q, levels[0])[0] == "ok"]
    got0 = {q for _, _, b, q in sc.scanned if b == 0}
    assert cands[SEGMENT] - cands[SEGMENT - 1] == SKIP and cands[SEGMENT + 1] - cands[SEGMENT - 1] == 2 * SKIP
    assert cands[SEGMENT - 1] in got0 and cands[SEGMENT] not in got0 and cands[SEGMENT + 1] in got0
    assert levels[1:3] == [0x3fff, 0x4000] and min(per_buffer[1:3]) > 200, (levels, per_buffer)
    for b in (1, 2):
        xb = sc.array(b).tolist()
        assert read(xb, 400, levels[b])[0] == "ok" and read(xb, 700, levels[b])[0] == "f1"
        assert (b, 400) in {(bb, p) for _, _, bb, p in sc.scanned}
    assert levels[4] == 0 and per_buffer[4] == 0 and per_buffer[5] == 1, (levels, per_buffer)
    assert read(sc.array(4).tolist(), 100, 0)[0] == "quiet"             # past both pulse tests; every window reads as a pulse
    x = sc.array(3).tolist()
    stages = [read(x, 70000 + 7 * i, levels[3])[0] for i in range(560)]
    assert set(stages) <= {"framing", "quiet", "noisy", "uncertain"}, set(stages)   # past F1 and F2, all fail the windows
    tile = [read(x, p, levels[3])[0] for p in range(70 * TILE, 71 * TILE)]
    assert sum(st not in ("f1", "f2") for st in tile) > 128                        # more than two rounds of 64 in one tile
    assert not [1 for _, _, b, p in sc.scanned if b == 3 and 69900 < p < 70000 + 7 * 560]   # (the train's end does decode)
    sc.levels = levels
    return sc


def waves_scene(nb):
    """Scene h: nb buffers, every one with replies at the first and last positions of its first and last tiles and of
    some between, and, in its first tile and in its last, a reply whose F1 is exactly at the buffer's own noise bound
    (m0 + m1 = 4 noise_level: delivered) and one a unit below it (rejected); neighbouring buffers hold different numbers
    of replies, so a level taken from the buffer in front or behind moves one of the two."""
    def build(levels):
        sc = AcScene(nb * CHUNK + 700, levels, seed=8)
        for b in range(nb):
            noise = sc.level(b)
            flat = 2 * noise + 400
            for tile, p in ((1, 0), (1, 1023), (3, 1023), (5, 0), (64, 0), (65, 1023), (126, 700), (127, 0)):
                sc.reply(b, tile * TILE + p, code=code_of(b * 8 + tile))
            for k in range(b % 5 * 6):                                     # 0 .. 24 more replies: another level
                sc.reply(b, 10 * TILE + 300 * k, code=code_of(k))
            for p0 in (400, 127 * TILE + 100):
                sc.reply(b, p0, code=0x0011, f1=(0, noise, 3 * noise, 0), f2=(0, flat, flat, 0))
                sc.reply(b, p0 + 200, code=0x0022, f1=(0, noise, 3 * noise - 1, 0), f2=(0, flat, flat, 0), expect="f1")
        return sc

    return settle(build)


def mixed_scene():
    """Scene i: Mode S frames (Scene.frame) among the replies, one of them over a reply in time.  The two passes are
    independent; a buffer's records are its Mode S messages, then its replies."""
    sc = AcScene(3 * CHUNK + 3000, seed=9)
    for b in range(3):
        for k in range(6):
            sc.reply(b, 2000 + 5000 * k, code=code_of(99 * b + k), spi=k == 2)
            sc.frame(capture_position(b, 4000 + 5000 * k), sub=k % 5, df=(17, 11)[k % 2], addr=0x400000 + 16 * b + k, high=3000)
    sc.reply(3, 1000, code=0x0007)
    sc.overlapped = sc.frame(capture_position(1, 2000 + 5000 * 3 - 100), sub=2, df=17, addr=0x4B0001, high=3000, accept=False)
    return sc.finish()


@functools.lru_cache(maxsize=None)
def scene(name, *args):
    """The scenes by name, built once."""
    return {"pulse": pulse_scene, "edge": edge_scene, "clock": clock_scene, "window": window_scene, "codes": codes_scene,
            "skip": skip_scene, "dense": dense_scene, "waves": waves_scene, "mixed": mixed_scene}[name](*args)
