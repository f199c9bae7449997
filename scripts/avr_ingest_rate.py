"""Lines/s and bytes/s of msd_accept_avr on a synthetic AVR text stream -- device-resident and from page-locked host
memory, at a few stream sizes -- the cost of one small call, and for comparison what a caller can do without it: a
msd_avr_parse_line per line on one host core (msd_avr_reader_feed: the line cutting and that call, the records into an
array) and one msd_accept_frames over the records.  Prints one JSON line.

    python scripts/avr_ingest_rate.py [--sizes-kib 64,1024,16384,65536] [--reps 3]
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
    rem = 0
    for byte in body:
        rem ^= byte << 16
        for _ in range(8):
            rem = ((rem << 1) ^ 0xFFF409) & 0xFFFFFF if rem & 0x800000 else (rem << 1) & 0xFFFFFF
    return rem


def with_parity(body, ap=0):
    return body + (crc24(body) ^ ap).to_bytes(3, "big")


def block(seed=1):
    """About 1 MiB of AVR lines: clean DF17 squitters of 2000 aircraft (5 % with one flipped bit), DF4 / DF20 replies
    of the same aircraft; '*' and '@' lines, LF and CRLF; 2 % junk lines."""
    rng = random.Random(seed)
    addrs = [rng.randrange(1, 1 << 24) for _ in range(2000)]
    out = bytearray()
    while len(out) < (1 << 20):
        a = rng.choice(addrs)
        r = rng.random()
        if r < 0.5:
            body = bytearray(with_parity(bytes([0x8D]) + a.to_bytes(3, "big") + bytes(rng.randrange(256) for _ in range(7))))
            if rng.random() < 0.05:
                bit = rng.randrange(40, 112)
                body[bit >> 3] ^= 0x80 >> (bit & 7)
        elif r < 0.8:
            body = with_parity(bytes([4 << 3, 0x00, 0x1F, 0xB8]), a)
        elif r < 0.98:
            body = with_parity(bytes([20 << 3, 0x00, 0x1F, 0xB8, 0x20, 0x05, 0x64, 0x1C, 0x30, 0x20, 0x00]), a)
        else:
            out += bytes(rng.choice(b"0123456789ABCDEF*;@ x") for _ in range(rng.randrange(40))) + b"\n"
            continue
        pre = b"*" if rng.random() < 0.7 else b"@%012X" % rng.randrange(1 << 48)
        out += pre + bytes(body).hex().upper().encode() + (b";\n" if rng.random() < 0.8 else b";\r\n")
    return bytes(out)


class ReaderState(C.Structure):  # host/msd_wire.h
    _fields_ = [("buf", C.c_uint8 * 257), ("len", C.c_size_t), ("discard", C.c_int), ("mode_ac", C.c_int),
                ("keep_timestamp", C.c_int), ("lines", C.c_uint64), ("frames", C.c_uint64),
                ("dropped_lines", C.c_uint64), ("long_lines", C.c_uint64)]


def best_of(reps, f):
    best, res = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-kib", default="64,1024,16384,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit the tree is (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as g
    pkg = g.load_package()
    sizes = [int(x) << 10 for x in args.sizes_kib.split(",")]
    blk = block()
    dem = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, message_capacity=max(sizes) // 16 + 4096)
    twin = pkg.Demodulator(fmt=pkg.FMT_UC8, nfix_crc=1, message_capacity=max(sizes) // 16 + 4096)
    dem.accept_avr(blk, 0)  # warm-up: kernels loaded, scratch allocated, the aircraft known
    host = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libmsd_host.so"))
    host.msd_avr_reader_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    host.msd_avr_reader_feed.restype = C.c_size_t
    host.msd_avr_reader_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    sink = C.cast(pkg.capi.lib().msd_array_sink, C.c_void_p)
    recs = np.zeros(max(sizes) // 7 + 2, dtype=pkg.capi.MESSAGE_DTYPE)
    recs.view(np.uint8)[:] = 0  # touched once, as a caller's buffer would be
    out = {"sizes": []}
    for n in sizes:
        stream = np.frombuffer((blk * (n // len(blk) + 1))[:n], dtype=np.uint8).copy()
        stream[-1] = 10
        dem.reset()
        twin.reset()
        dem.accept_avr(blk, 0)
        twin.accept_frames(recs[:0], 0)
        dev = torch.from_numpy(stream).to("cuda:0")
        torch.cuda.synchronize()
        pinned = dem.host_buffer(n)
        pinned[:] = stream
        before = dem.avr_stats()
        t_dev, got = best_of(args.reps, lambda: dem.accept_avr(dev, 1))
        lines = (dem.avr_stats()["lines"] - before["lines"]) // args.reps
        t_pin, _ = best_of(args.reps, lambda: dem.accept_avr(pinned, 2))

        def caller():
            r = ReaderState()
            host.msd_avr_reader_init(C.byref(r), 0, 0)
            st = pkg.capi._SinkState(recs.ctypes.data, recs.size, 0)
            t0 = time.perf_counter()
            k = host.msd_avr_reader_feed(C.byref(r), stream.ctypes.data, n, sink, C.byref(st))
            t1 = time.perf_counter()
            res = twin.accept_frames(recs[:k], 2)
            return t1 - t0, time.perf_counter() - t1, len(res)

        t_host, parts = best_of(args.reps, caller)
        row = {"bytes": n, "lines": int(lines), "accepted": int(len(got)),
               "device_resident": {"s": round(t_dev, 5), "GBps": round(n / t_dev / 1e9, 3),
                                   "Mlines_per_s": round(lines / t_dev / 1e6, 2)},
               "host_pinned": {"s": round(t_pin, 5), "GBps": round(n / t_pin / 1e9, 3),
                               "Mlines_per_s": round(lines / t_pin / 1e6, 2)},
               "parse_line_loop_then_accept_frames": {"s": round(t_host, 5), "GBps": round(n / t_host / 1e9, 3),
                                                      "Mlines_per_s": round(lines / t_host / 1e6, 2),
                                                      "parse_s": round(parts[0], 5), "accept_frames_s": round(parts[1], 5),
                                                      "accepted": parts[2]},
               "speedup_host_pinned": round(t_host / t_pin, 2), "speedup_device_resident": round(t_host / t_dev, 2)}
        out["sizes"].append(row)
        del dev

    # small calls: what one call costs whatever it carries (a socket read handed over as it comes)
    small = np.frombuffer(blk[: 4096 * 201], dtype=np.uint8).copy()
    times = []
    for k in range(201):
        t0 = time.perf_counter()
        dem.accept_avr(small[4096 * k: 4096 * (k + 1)], 3)
        times.append(time.perf_counter() - t0)
    times = sorted(times[1:])
    out["calls_of_4_KiB_from_host"] = {"us_p50": round(1e6 * times[len(times) // 2], 1),
                                       "us_p99": round(1e6 * times[int(len(times) * 0.99)], 1),
                                       "MBps": round(4096 / times[len(times) // 2] / 1e6, 2)}
    out["what"] = ("parse_line_loop_then_accept_frames: msd_avr_reader_feed on one core (the line cutting and one "
                   "msd_avr_parse_line per line, the records into an array), then one msd_accept_frames over them")
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
