"""Every one- and two-bit error pattern, once: constructed scenes (mag_scenes.Scene) whose CRC repair has a designed
answer.  Plain numpy; no product code and no oracle.  The only thing taken from another reading is the list of
syndromes --aggressive corrects, indep_demod.error_table (crc.c:184-350 restated), and the checksum of received bytes.

Every frame k of a scene starts at sub-sample tick k % 5 with pulse level (20000, 65535, 1200, 30000)[k % 4] (the cycles
of mag_scenes.tie_scene) and carries `pat`, the tuple of bits flipped in it.

  * long_scene(): 112-bit frames 320 samples apart.  One clean DF17 of A in front (it adds A to the ICAO filter);
    then, for A and for an address B that is never sent clean, a DF17 with every single flip 0..111 and every pair from
    5..111 (112 + 5671 patterns per address); then DF18 of A with every single flip and every 7th pair.
  * short_scene(): DF11 frames 176 samples apart.  One clean DF11 of A in front; then four blocks -- A with IID 0, A
    with IID 5, unknown addresses with IID 0, unknown addresses with IID 5 (a fresh address per frame) -- each with
    every single flip 0..55 and every pair from 5..55 (56 + 1275 patterns).

design(scene, nfix) fills in what depends on the repair level: each frame's `accept`, the bytes it is delivered with
(`bytes`) and its `corrected` count, by the closed-form rules below; scene.expected() then counts with them.

Long frames (mode_s.c:489-520, 266-281, 386-399): a pattern is repaired iff it has at most nfix bits, none of them in
the DF field (bits 0..4: crc.c:214 leaves them out of the tables), and it is a single or one of the pairs that
--aggressive keeps; a repaired frame is accepted iff no flipped bit lies in the address (8..31) or the address is in
the filter (it is A).  Delivered: the clean frame, correctedbits = len(pat).

DF11 (mode_s.c:355-375, 449-465), on the received bytes rx with crc = checksum(rx): not a DF11 any more: never.
crc & 0xffff80 == 0: accepted as received, flipped parity bits and all, iff crc & 0x7f == 0 or the address is in the
filter.  Otherwise crc & 0xffff80 looked up in the 56-bit table: an entry of exactly one bit is flipped in rx and the
frame accepted iff the address it now holds is in the filter, correctedbits 1 -- often not the frame that was sent,
since the mask leaves syndromes that name a different bit.  A DF11 is never repaired in two bits.

The filter the rules ask is a set carried from frame to frame: A from the clean frame in front, and whatever a frame
accepted without repair adds (a DF17; a DF11 whose crc & 0x7f is 0 -- a flipped pair that cancels IID 5 reads as one).
"""
import functools
import itertools

import numpy as np

import indep_demod
import indep_signal
import mag_scenes as ms

A = 0x4840D6
B = 0xA0C1E5
UNKNOWN = 0x200000          # the unknown DF11 blocks: address UNKNOWN + k of frame k
LEVELS = (20000, 65535, 1200, 30000)
LONG_PITCH, SHORT_PITCH = 320, 176
FIRST = 1000                # start sample of a scene's first frame
DF18_EVERY = 7
# The payloads are random, and for about every second payload --aggressive reads a repairable frame into the sliced tail
# of a rejected frame of the long scene (one or two messages among 7000, as magnitudes or as UC8; seeds 41 .. 48 were
# tried).  With these seeds nothing but the placed frames is delivered, at every level, as magnitudes and as UC8:
# tests/test_repair_scenes.py holds the oracle to that.
LONG_SEED, SHORT_SEED = 44, 43

SINGLES_112, PAIRS_112 = 107, 3724
SINGLES_56, PAIRS_56 = 51, 1275      # every 56-bit pair is kept (and none is ever applied to a DF11)


def patterns(nbits, every=1):
    """Every single flip 0 .. nbits - 1, then every `every`-th pair from 5 .. nbits - 1."""
    pairs = list(itertools.combinations(range(5, nbits), 2))
    return [(i,) for i in range(nbits)] + pairs[::every]


def correctable_pairs(nbits):
    return {v for v in indep_demod.error_table(nbits, 2).values() if len(v) == 2}


def _body(rng, df, addr, nbits):
    """DF, CA / CF and the address, then random ME bits (none for a DF11)."""
    return np.concatenate([indep_signal.to_bits(df, 5), rng.integers(0, 2, 3, dtype=np.uint8),
                           indep_signal.to_bits(addr, 24), rng.integers(0, 2, nbits - 56, dtype=np.uint8)])


class RepairScene(ms.Scene):
    """A Scene that remembers how it was put together, so that it can be rendered again at another level."""

    def __init__(self, n, pitch):
        super().__init__(n)
        self.pitch = pitch
        self.specs = []      # (clean bits, pat, properties) per frame, in order
        self.uc8 = None      # to_uc8()'s rendering

    def add(self, clean, pat, level=None, **props):
        k = len(self.frames)
        f = self.frame(FIRST + self.pitch * k, sub=k % 5, bits=clean, flip=pat,
                       high=LEVELS[k % 4] if level is None else level)
        f["addr"] = int(np.packbits(clean[8:32]).tobytes().hex(), 16)
        f.update(pat=tuple(pat), clean=f["bytes"], rx=ms.bits_to_bytes(f["bits"]), corrected=0, **props)
        self.specs.append((clean, tuple(pat), props))
        return f


def _render(plan, pitch, level=None):
    n = FIRST + pitch * len(plan) + 2 * pitch
    sc = RepairScene(n, pitch)
    for clean, pat, props in plan:
        sc.add(clean, pat, level, **props)
    return sc


def _long_plan(seed=LONG_SEED):
    rng = np.random.default_rng(seed)
    plan = []
    a17 = ms.frame_bits(rng, 17, A, body=_body(rng, 17, A, 112))
    b17 = ms.frame_bits(rng, 17, B, body=_body(rng, 17, B, 112))
    a18 = ms.frame_bits(rng, 18, A, body=_body(rng, 18, A, 112))
    plan.append((a17, (), dict(block="A clean")))
    for name, clean, every in (("A DF17", a17, 1), ("B DF17", b17, 1), ("A DF18", a18, DF18_EVERY)):
        for pat in patterns(112, every):
            plan.append((clean, pat, dict(block=name)))
    return plan


def _short_plan(seed=SHORT_SEED):
    rng = np.random.default_rng(seed)
    plan = []
    a0 = ms.frame_bits(rng, 11, A, body=_body(rng, 11, A, 56))
    a5 = ms.frame_bits(rng, 11, A, parity_xor=5, body=a0[:32])
    plan.append((a0, (), dict(block="A clean")))
    for name, addr, iid in (("A IID 0", A, 0), ("A IID 5", A, 5), ("unknown IID 0", None, 0), ("unknown IID 5", None, 5)):
        for pat in patterns(56):
            if addr is None:
                clean = ms.frame_bits(rng, 11, 0, parity_xor=iid, body=_body(rng, 11, UNKNOWN + len(plan), 56))
            else:
                clean = a5 if iid else a0
            plan.append((clean, pat, dict(block=name)))
    return plan


@functools.lru_cache(maxsize=None)
def long_scene():
    return _render(_long_plan(), LONG_PITCH)


@functools.lru_cache(maxsize=None)
def short_scene():
    return _render(_short_plan(), SHORT_PITCH)


def thinned(scene, every):
    """The scene's first frame (it adds A) and every `every`-th pattern behind it, as a scene of its own."""
    plan = scene.specs[:1] + scene.specs[1::every]
    return _render(plan, scene.pitch)


# ---- the designed answer --------------------------------------------------------------------------------------------------

def _flip(rx, bit):
    out = bytearray(rx)
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(out)


def _address(msg):
    return (msg[1] << 16) | (msg[2] << 8) | msg[3]


def decide_long(f, nfix, known, pairs):
    """(accept, bytes, corrected) of a 112-bit frame of this module, by its pattern."""
    pat = f["pat"]
    if not pat:
        return True, f["clean"], 0
    repaired = len(pat) <= nfix and min(pat) >= 5 and (len(pat) == 1 or pat in pairs)
    accept = repaired and (not any(8 <= b <= 31 for b in pat) or f["addr"] in known)
    return accept, f["clean"], len(pat)


def decide_short(f, nfix, known, demod=True):
    """(accept, bytes, corrected) of a DF11 of this module, by its received bytes.  demod=False: Beast / AVR input, which
    goes to decodeModesMessage without scoreModesMessage in front of it (net_io.c:1573-1627) -- there a frame with
    crc & 0xffff80 == 0 is accepted whatever its IID and address."""
    rx = f["rx"]
    if rx[0] >> 3 != 11:
        return False, rx, 0
    crc = indep_demod.checksum(rx, 56)
    if crc & 0xFFFF80 == 0:
        return not demod or (crc & 0x7F) == 0 or _address(rx) in known, rx, 0
    table = indep_demod.error_table(56, nfix)
    entry = table.get(crc & 0xFFFF80) if table else None
    if entry is None or len(entry) != 1:
        return False, rx, 0
    fixed = _flip(rx, entry[0])
    return _address(fixed) in known, fixed, 1


def design_frames(frames, nfix, known=None, demod=True):
    """Fill in accept / bytes / corrected of the frames, in order, against the filter `known` (a set; updated).
    demod=False: the frames arrive as Beast / AVR input (decide_short)."""
    known = set() if known is None else known
    pairs = correctable_pairs(112)
    for f in frames:
        if f["msgbits"] == 112:
            accept, data, corrected = decide_long(f, nfix, known, pairs)
        else:
            accept, data, corrected = decide_short(f, nfix, known, demod)
        f["accept"], f["bytes"], f["corrected"] = bool(accept), data, corrected
        if accept and corrected == 0 and (data[0] >> 3 == 17 or (data[0] >> 3 == 11 and indep_demod.checksum(data, 56) & 0x7F == 0)):
            known.add(_address(data))
    return known


def design(scene, nfix):
    """The scene's frames with the answer of repair level nfix (0: --no-fix, 1: --fix, 2: --aggressive) filled in."""
    design_frames(scene.frames, nfix)
    return scene


def accepted(scene):
    return [f for f in scene.frames if f["accept"]]


def histogram(scene):
    """demod_accepted as designed: accepted frames per corrected-bit count."""
    out = [0, 0, 0]
    for f in accepted(scene):
        out[f["corrected"]] += 1
    return out


# ---- UC8 rendering -------------------------------------------------------------------------------------------------------

UC8_EXTRAS = 5   # messages beyond the designed ones a UC8 replay may deliver (sliced tails of rejected frames)


def to_uc8(scene):
    """The scene's frames at one level, 65535, as whole buffers of UC8: I = 128 + round(mag / 65535 * 127), Q = 128.
    Rendered once per scene."""
    if getattr(scene, "uc8", None) is None:
        flat = _render(scene.specs, scene.pitch, level=65535)
        nbuf = -(-flat.n // ms.CHUNK)
        mag = np.zeros(nbuf * ms.CHUNK, dtype=np.float64)
        mag[:flat.n] = flat.mag
        iq = np.full(2 * mag.size, 128, dtype=np.uint8)
        iq[0::2] = (128 + np.round(mag / 65535.0 * 127.0)).astype(np.uint8)
        scene.uc8 = iq
    return scene.uc8


def check_uc8(msgs, scene):
    """Every designed (bytes, correctedbits) appears, in order, and at most UC8_EXTRAS messages beyond them."""
    got = [(bytes(m["msg"][: int(m["msgbits"]) // 8]), int(m["correctedbits"])) for m in msgs]
    want = [(f["bytes"], f["corrected"]) for f in accepted(scene)]
    k = 0
    for g in got:
        if k < len(want) and g == want[k]:
            k += 1
    assert k == len(want), ("designed message missing", k, len(want), want[k][0].hex(), want[k][1])
    assert len(got) - len(want) <= UC8_EXTRAS, (len(got), len(want))
