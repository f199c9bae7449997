"""Frames/s and GB/s of msd_accept_beast on a synthetic Beast stream: device-resident, from page-locked host memory, and
msd_beast_reader_feed (framing only, no acceptance, no sink) on one core for comparison.  Prints one JSON line.

    python scripts/beast_ingest_rate.py [--mib 1024] [--host-mib 64] [--reps 3]

The host comparison is framing alone: the project has no host restatement of the acceptance in C (the checker in
tests/remote_decode.py is Python), so the host side is measured without any CRC or filter work.  Each call's fixed cost
(filter snapshot upload, about 20 launches, 3 synchronisations) is measured too, on 4 KiB calls.
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def crc24(body):
    """modesChecksum remainder of body + three zero bytes (crc.c:31,67-82), by long division."""
    rem = 0
    for byte in body:
        rem ^= byte << 16
        for _ in range(8):
            rem = ((rem << 1) ^ 0xFFF409) & 0xFFFFFF if rem & 0x800000 else (rem << 1) & 0xFFFFFF
    return rem


def with_parity(body, ap=0):
    """body + the parity bytes that make the syndrome `ap` (0: a clean PI field, else the address of an AP reply)."""
    return body + (crc24(body) ^ ap).to_bytes(3, "big")


def beast(type_byte, payload, ts, signal):
    """0x1A, type, 6-byte timestamp, signal byte, payload; every 0x1A after the type doubled (net_io.c:795-830)."""
    body = ts.to_bytes(6, "big") + bytes([signal]) + bytes(payload)
    return b"\x1a" + bytes([type_byte]) + body.replace(b"\x1a", b"\x1a\x1a")


def block(seed=1):
    """About 1 MiB of Beast frames: clean DF17 squitters of 2000 aircraft (5 % with one flipped bit), DF4 / DF20
    replies of the same aircraft, and 2 % garbage runs."""
    rng = random.Random(seed)
    addrs = [rng.randrange(1, 1 << 24) for _ in range(2000)]
    out = bytearray()
    while len(out) < (1 << 20):
        a = rng.choice(addrs)
        ts = rng.randrange(1 << 48)
        r = rng.random()
        if r < 0.5:
            body = bytearray(with_parity(bytes([0x8D]) + a.to_bytes(3, "big") + bytes(rng.randrange(256) for _ in range(7))))
            if rng.random() < 0.05:
                bit = rng.randrange(40, 112)
                body[bit >> 3] ^= 0x80 >> (bit & 7)
            out += beast(ord("3"), body, ts, rng.randrange(256))
        elif r < 0.8:
            out += beast(ord("2"), with_parity(bytes([4 << 3, 0x00, 0x1F, 0xB8]), a), ts, rng.randrange(256))
        elif r < 0.98:
            out += beast(ord("3"), with_parity(bytes([20 << 3, 0x00, 0x1F, 0xB8, 0x20, 0x05, 0x64, 0x1C, 0x30, 0x20, 0x00]), a),
                         ts, rng.randrange(256))
        else:
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(40)))
    return bytes(out)


class BeastReader(C.Structure):  # host/msd_wire.h
    _fields_ = [("buf", C.c_uint8 * 256), ("len", C.c_size_t), ("mode_ac", C.c_int), ("frames", C.c_uint64),
                ("modeac_ignored", C.c_uint64), ("other_frames", C.c_uint64), ("garbage_bytes", C.c_uint64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--host-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit the tree is (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    blk = np.frombuffer(block(), dtype=np.uint8)
    reps = (args.mib << 20) // blk.size
    stream = np.tile(blk, reps)
    n = stream.size
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, message_capacity=(args.mib << 20) // 16)  # frames take 21 bytes on average
    first = dem.accept_beast(blk, 0)  # warm-up: kernels loaded, scratch allocated, the aircraft known
    frames_per_block = dem.remote_stats()["frames"]
    out = {"stream_bytes": int(n), "frames": int(frames_per_block * reps), "accepted_first_block": int(len(first))}

    dev = torch.from_numpy(stream).to("cuda:0")
    torch.cuda.synchronize()
    best = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = dem.accept_beast(dev, 1)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["device_resident"] = {"s": round(best, 4), "GBps": round(n / best / 1e9, 3),
                              "Mframes_per_s": round(out["frames"] / best / 1e6, 2), "accepted": int(len(got))}
    pinned = dem.host_buffer(n)
    pinned[:] = stream
    best = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = dem.accept_beast(pinned, 2)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["host_pinned"] = {"s": round(best, 4), "GBps": round(n / best / 1e9, 3),
                          "Mframes_per_s": round(out["frames"] / best / 1e6, 2), "accepted": int(len(got))}

    # small calls: what one call costs whatever it carries (a socket read handed over as it comes)
    small = np.ascontiguousarray(stream[: 4096 * 201])
    times = []
    for k in range(201):
        t0 = time.perf_counter()
        dem.accept_beast(small[4096 * k: 4096 * (k + 1)], 3)
        times.append(time.perf_counter() - t0)
    times = sorted(times[1:])
    out["calls_of_4_KiB_from_host"] = {"us_p50": round(1e6 * times[len(times) // 2], 1),
                                       "us_p99": round(1e6 * times[int(len(times) * 0.99)], 1),
                                       "MBps": round(4096 / times[len(times) // 2] / 1e6, 2)}

    host = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    sink_t = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
    host.msd_beast_reader_init.argtypes = [C.c_void_p, C.c_int]
    host.msd_beast_reader_feed.restype = C.c_size_t
    host.msd_beast_reader_feed.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, sink_t, C.c_void_p]
    hn = min(n, args.host_mib << 20)
    hbuf = stream[:hn].tobytes()
    r = BeastReader()
    host.msd_beast_reader_init(C.byref(r), 0)
    t0 = time.perf_counter()
    host.msd_beast_reader_feed(C.byref(r), hbuf, hn, sink_t(), None)
    dt = time.perf_counter() - t0
    out["host_reader_framing_one_core"] = {"bytes": hn, "s": round(dt, 4), "GBps": round(hn / dt / 1e9, 3),
                                           "Mframes_per_s": round(r.frames / dt / 1e6, 2),
                                           "what": "msd_beast_reader_feed with no sink: framing only, no CRC, no "
                                                   "filter; a host acceptance would add to this"}
    out["commit"] = args.commit
    if out["commit"] is None:
        try:
            out["commit"] = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                           text=True).stdout.strip() or None
        except OSError:
            pass
    print(json.dumps(out))


if __name__ == "__main__":
    main()
