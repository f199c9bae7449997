"""Call time of a receiver group (msd_group_*) against one Demodulator per receiver; writes
profiles/receiver_group_rate.json.

    python scripts/receiver_group_rate.py [--reps 5] [--out profiles/receiver_group_rate.json]

A K-entry call takes one 131072-sample UC8 buffer from each of K receivers.  Real time for one receiver is
131072 / 2.4e6 = 54.6 ms per buffer, so a call of time t sustains K * 54.6 ms / t receivers.  Messages are
not handed to Python (deliver=False); the counters are.  The kernel trace of the K = 1024 call is a separate run:
rocprofv3 --kernel-trace --stats -- python scripts/receiver_group_rate.py --only 1024 --reps 1
(profiles/receiver_group_k1024_kernel_stats.csv).

    python scripts/receiver_group_rate.py --mixed [--reps 20]

times the K = 1024 call with per-receiver options (thresholds spread over 40..400, repair levels 0 / 1 / 2 mixed)
beside the same call with every receiver at the group's defaults, alternating, in one process; writes
profiles/receiver_group_options_rate.json.

    python scripts/receiver_group_rate.py --modeac [--reps 20]

times the K = 1024 call with Mode A/C off for every receiver, on for every other one, and on for all, alternating, in
one process, over a capture with 2000 Mode A/C replies a second; writes profiles/receiver_group_modeac_rate.json.  Its
kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/receiver_group_rate.py --modeac --reps 3 --out
/tmp/x.json (profiles/receiver_group_modeac_k1024_kernel_stats.csv).

    python scripts/receiver_group_rate.py --fields [--reps 20]

times the K = 1024 call three ways, alternating, in one process: the plain call on a group made without
MSD_CFG_DECODE_FIELDS, the plain call on a group made with it, and the fields call (msd_group_submit_*_fields) on
that group, over a capture with 2000 Mode A/C replies a second and Mode A/C on for every other receiver; writes
profiles/receiver_group_fields_rate.json.  Its kernel trace: rocprofv3 --kernel-trace --stats -- python
scripts/receiver_group_rate.py --fields --reps 3 --out /tmp/x.json
(profiles/receiver_group_fields_k1024_kernel_stats.csv).

    python scripts/receiver_group_rate.py --wire [--reps 20]

times the K = 1024 call three ways, alternating, in one process, over the --fields capture and with Mode A/C on for every
other receiver: the plain call with a C sink that only counts; the plain call with a C sink that runs
msd_beast_frame_out on every message into one array -- the only way to these bytes without the wire entries --; and the
wire call (msd_group_submit_*_wire, Beast) with a C sink that adds up the sizes it is handed.  The three sinks are
compiled by the script (gcc) against libmsd_host.so.  Writes profiles/receiver_group_wire_rate.json.  Its kernel trace:
rocprofv3 --kernel-trace --stats -- python scripts/receiver_group_rate.py --wire --reps 3 --out /tmp/x.json
(profiles/receiver_group_wire_k1024_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 131072


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--modeac", action="store_true")
    ap.add_argument("--fields", action="store_true")
    ap.add_argument("--wire", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "receiver_group_options_rate.json" if a.mixed else
                             "receiver_group_modeac_rate.json" if a.modeac else
                             "receiver_group_fields_rate.json" if a.fields else
                             "receiver_group_wire_rate.json" if a.wire else "receiver_group_rate.json")
    import __graft_entry__ as g
    pkg = g.load_package()
    import torch
    capi, siggen = pkg.capi, pkg.siggen
    base = siggen.generate(siggen.make_cfg(seed=17, msgs_per_sec=3000, n_aircraft=60, ac_per_sec=2000 if a.modeac or a.fields or a.wire else 0),
                           64 * CHUNK)
    ks = [a.only] if a.only else [1, 16, 256, 1024]
    kmax = max(ks)
    host = np.empty(kmax * CHUNK * 2, dtype=np.uint8)
    for r in range(kmax):
        host[r * CHUNK * 2:(r + 1) * CHUNK * 2] = base[(r % 64) * CHUNK * 2:((r % 64) + 1) * CHUNK * 2]
    dev = torch.from_numpy(host).cuda()
    if a.mixed:
        return mixed(a, capi, dev, host)
    if a.modeac:
        return modeac(a, capi, dev, host)
    if a.fields:
        return fields(a, capi, dev, host)
    if a.wire:
        return wire(a, capi, dev, host)
    res = {"buffer_samples": CHUNK, "format": "uc8", "reps": a.reps, "group": {}}
    for k in ks:
        grp = capi.ReceiverGroup(k, fmt=capi.FMT_UC8)
        row = {}
        for where, iq in (("device", dev), ("host", host)):
            grp.submit(iq, list(range(k)), deliver=False)  # warm-up: arenas, threads, first-touch
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                grp.submit(iq, list(range(k)), deliver=False)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            row[where] = {"call_ms_median": t * 1e3, "call_ms_all": [x * 1e3 for x in ts],
                          "gsamples_per_s": k * CHUNK / t / 1e9, "receivers_real_time": k * (CHUNK / 2.4e6) / t}
        t = grp.timing()  # (the group keeps no kernel times: the rocprofv3 run has them)
        row["timing"] = {k: t[k] for k in ("hits", "tries", "reruns", "resolve_passes", "resolve_fallback")}
        res["group"][str(k)] = row
        grp.close()
        print(k, json.dumps({w: round(row[w]["call_ms_median"], 3) for w in ("device", "host")}), flush=True)
    if not a.only:
        res["separate_demodulators"] = {}
        for k in (16, 64):
            ds = [capi.Demodulator(fmt=capi.FMT_UC8, flags=0) for _ in range(k)]
            for i, d in enumerate(ds):  # warm-up
                d.submit_device(dev.data_ptr() + i * CHUNK * 2, CHUNK, last=False)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for i, d in enumerate(ds):
                    d.launch_device(dev.data_ptr() + i * CHUNK * 2, CHUNK, last=False)
                for d in ds:
                    d.collect(copy=False)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            res["separate_demodulators"][str(k)] = {"round_ms_median": t * 1e3, "gsamples_per_s": k * CHUNK / t / 1e9}
            for d in ds:
                d.close()
            print("separate", k, round(t * 1e3, 3), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def mixed_options(k):
    """receiver r: threshold 40 + (97 r) % 361, spread over 40..400; repair level r % 3"""
    return [(40 + (97 * r) % 361, r % 3) for r in range(k)]


def mixed(a, capi, dev, host):
    k = 1024
    groups = {"uniform": capi.ReceiverGroup(k, fmt=capi.FMT_UC8), "mixed": capi.ReceiverGroup(k, fmt=capi.FMT_UC8)}
    opts = mixed_options(k)
    for r, (t, n) in enumerate(opts):
        groups["mixed"].set_receiver_options(r, preamble_threshold=t, nfix_crc=n)
    res = {"buffer_samples": CHUNK, "format": "uc8", "receivers": k, "reps": a.reps,
           "mixed_options": "threshold 40 + (97 r) % 361, nfix_crc r % 3", "calls": {}}
    alternate(a, k, groups, dev, host, res)


def modeac(a, capi, dev, host):
    k = 1024
    groups = {name: capi.ReceiverGroup(k, fmt=capi.FMT_UC8) for name in ("off", "half", "all")}
    for r in range(k):
        if r % 2 == 0:
            groups["half"].set_receiver_mode_ac(r, 1)
        groups["all"].set_receiver_mode_ac(r, 1)
    res = {"buffer_samples": CHUNK, "format": "uc8", "receivers": k, "reps": a.reps,
           "capture": "siggen seed 17, 3000 Mode S and 2000 Mode A/C replies a second",
           "mode_ac": "off: none, half: even receivers, all: every receiver", "calls": {}}
    alternate(a, k, groups, dev, host, res, modeac=True)


def fields(a, capi, dev, host):
    k = 1024
    flagged = capi.ReceiverGroup(k, fmt=capi.FMT_UC8, flags=capi.CFG_DECODE_FIELDS)
    groups = {"plain": capi.ReceiverGroup(k, fmt=capi.FMT_UC8), "plain_on_fields_group": flagged, "fields": flagged}
    for grp in (groups["plain"], flagged):
        for r in range(0, k, 2):
            grp.set_receiver_mode_ac(r, 1)
    res = {"buffer_samples": CHUNK, "format": "uc8", "receivers": k, "reps": a.reps,
           "capture": "siggen seed 17, 3000 Mode S and 2000 Mode A/C replies a second; Mode A/C on for even receivers",
           "groups": "plain: made without MSD_CFG_DECODE_FIELDS; plain_on_fields_group / fields: one group made with it, "
                     "through msd_group_submit_* and msd_group_submit_*_fields; no sink in either (deliver=False)",
           "calls": {}}
    alternate(a, k, groups, dev, host, res, modeac=True, fields_of=("fields",))


WIRE_SINKS_C = r"""
#include <stddef.h>
#include <stdint.h>
size_t msd_beast_frame_out(const void *mm, int net_verbatim, uint8_t *out);
struct state { uint8_t *buf; size_t used, cap; uint64_t messages, calls; };
void count_sink(uint32_t receiver, const void *mm, void *user)
{
    struct state *s = user;
    (void)receiver; (void)mm;
    s->calls++;
}
void beast_sink(uint32_t receiver, const void *mm, void *user)
{
    struct state *s = user;
    (void)receiver;
    s->calls++;
    if (s->used + 44 <= s->cap) {
        const size_t n = msd_beast_frame_out(mm, 0, s->buf + s->used);
        s->used += n;
        s->messages += n != 0;
    }
}
void wire_sink(uint32_t receiver, const uint8_t *bytes, size_t nbytes, uint32_t nmessages, void *user)
{
    struct state *s = user;
    (void)receiver; (void)bytes;
    s->calls++;
    s->used += nbytes;
    s->messages += nmessages;
}
"""


def wire(a, capi, dev, host):
    import ctypes as C
    import subprocess
    import tempfile
    k = 1024
    libdir = os.path.dirname(capi.LIB_PATH)
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "sinks.c"), "w") as f:
        f.write(WIRE_SINKS_C)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", os.path.join(tmp, "sinks.so"), os.path.join(tmp, "sinks.c"),
                           "-L" + libdir, "-lmsd_host", "-Wl,-rpath," + libdir])
    sinks = C.CDLL(os.path.join(tmp, "sinks.so"))

    class State(C.Structure):
        _fields_ = [("buf", C.c_void_p), ("used", C.c_size_t), ("cap", C.c_size_t), ("messages", C.c_uint64),
                    ("calls", C.c_uint64)]

    out = np.zeros(64 << 20, dtype=np.uint8)
    L = capi._group_lib()
    groups = {name: capi.ReceiverGroup(k, fmt=capi.FMT_UC8) for name in ("plain", "plain_host_beast", "wire")}
    for grp in groups.values():
        for r in range(0, k, 2):
            grp.set_receiver_mode_ac(r, 1)
    entries = (capi.GroupEntry * k)(*[capi.GroupEntry(r, 0, 0) for r in range(k)])
    fn = {n: C.cast(getattr(sinks, n), C.c_void_p) for n in ("count_sink", "beast_sink", "wire_sink")}
    last = {}

    def call(name, where):
        st = State(out.ctypes.data, 0, out.size, 0, 0)
        iq = C.c_void_p(dev.data_ptr()) if where == "device" else host.ctypes.data
        h = groups[name]._h
        if name == "wire":
            f = L.msd_group_submit_device_wire if where == "device" else L.msd_group_submit_host_wire
            rc = f(h, iq, entries, k, capi.WIRE_BEAST, 0, fn["wire_sink"], C.byref(st))
        else:
            f = L.msd_group_submit_device if where == "device" else L.msd_group_submit_host
            rc = f(h, iq, entries, k, fn["count_sink" if name == "plain" else "beast_sink"], C.byref(st))
        if rc:
            raise RuntimeError(f"{name}: {rc}")
        last[name] = {"sink_calls": st.calls, "bytes": st.used, "messages": st.messages}

    res = {"buffer_samples": CHUNK, "format": "uc8", "receivers": k, "reps": a.reps,
           "capture": "siggen seed 17, 3000 Mode S and 2000 Mode A/C replies a second; Mode A/C on for even receivers",
           "calls_timed": "plain: msd_group_submit_* with a sink that counts; plain_host_beast: the same with a sink that runs "
                          "msd_beast_frame_out into one array; wire: msd_group_submit_*_wire (Beast) with a sink that adds up "
                          "the sizes (it does not copy the bytes)", "calls": {}}
    for where in ("device", "host"):
        ts = {name: [] for name in groups}
        for name in groups:
            call(name, where)  # warm-up
        for _ in range(a.reps):  # alternating, so that drift of the box falls on all alike
            for name in groups:
                t0 = time.perf_counter()
                call(name, where)
                ts[name].append(time.perf_counter() - t0)
        for name, v in ts.items():
            t = float(np.median(v))
            res["calls"].setdefault(name, {})[where] = {
                "call_ms_median": t * 1e3, "call_ms_min": min(v) * 1e3, "call_ms_max": max(v) * 1e3,
                "call_ms_all": [x * 1e3 for x in v], "receivers_real_time": k * (CHUNK / 2.4e6) / t, "last_call": last[name]}
        print(where, json.dumps({n: round(res["calls"][n][where]["call_ms_median"], 3) for n in groups}), flush=True)
    for name, grp in groups.items():
        t = grp.timing()
        res["calls"][name]["timing"] = {x: t[x] for x in ("hits", "tries", "reruns", "resolve_passes", "resolve_fallback")}
        grp.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


def alternate(a, k, groups, dev, host, res, modeac=False, fields_of=()):
    for where, iq in (("device", dev), ("host", host)):
        ts = {name: [] for name in groups}
        for name, grp in groups.items():
            grp.submit(iq, list(range(k)), deliver=False, fields=name in fields_of)  # warm-up
        for _ in range(a.reps):  # alternating, so that drift of the box falls on both alike
            for name, grp in groups.items():
                t0 = time.perf_counter()
                grp.submit(iq, list(range(k)), deliver=False, fields=name in fields_of)
                ts[name].append(time.perf_counter() - t0)
        for name, v in ts.items():
            t = float(np.median(v))
            res["calls"].setdefault(name, {})[where] = {
                "call_ms_median": t * 1e3, "call_ms_min": min(v) * 1e3, "call_ms_all": [x * 1e3 for x in v],
                "gsamples_per_s": k * CHUNK / t / 1e9, "receivers_real_time": k * (CHUNK / 2.4e6) / t}
        print(where, json.dumps({n: round(res["calls"][n][where]["call_ms_median"], 3) for n in groups}), flush=True)
    for name, grp in groups.items():
        t = grp.timing()
        res["calls"][name]["timing"] = {x: t[x] for x in ("hits", "tries", "reruns", "resolve_passes", "resolve_fallback")}
        res["calls"][name]["accepted"] = int(sum(sum(grp.stats(r)["demod_accepted"]) for r in range(k)))
        if modeac:
            res["calls"][name]["demod_modeac"] = int(sum(grp.stats(r)["demod_modeac"] for r in range(k)))
    for grp in groups.values():
        grp.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
