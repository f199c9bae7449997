"""Call time of the fields and wire calls of a group's Beast input (msd_group_accept_beast_fields,
msd_group_accept_beast_wire) against the plain msd_group_accept_beast call of the same process; writes
profiles/group_remote_out_rate.json.

    python scripts/group_remote_out_rate.py [--receivers 1024] [--bytes 4096] [--reps 20] [--format 0] [--verbatim]

Workload: that of scripts/group_beast_rate.py -- K = 1024 receivers, 4 KiB of a Beast stream each per round, cut at
arbitrary byte positions.  Three groups of one configuration (the fields one with MSD_CFG_DECODE_FIELDS) get the same
bytes with the same now_ms, one round of each call alternating in one process, from device and from host memory; no
sink is passed, so the time is the library's; the remote counters of the three groups are compared at the end.  The
plain call's time is also what to hold against scripts/group_beast_rate.py's figure for the parent commit.

The per-kernel table is a separate run:
    rocprofv3 --kernel-trace --stats -- python scripts/group_remote_out_rate.py --reps 3 --out /tmp/x.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from group_beast_rate import beast_stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receivers", type=int, default=1024)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--format", type=int, default=0, help="MSD_WIRE_BEAST 0, MSD_WIRE_AVR 1, MSD_WIRE_AVR_MLAT 2")
    ap.add_argument("--verbatim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_remote_out_rate.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg, O = g.load_package(), g.load_oracle()
    import torch
    capi = pkg.capi
    K, B = a.receivers, a.bytes
    rounds = a.reps + 1  # one warm-up round: scratch, first touch
    streams = [beast_stream(pkg, O, 100 + s, rounds * B) for s in range(8)]
    host = np.empty((rounds, K, B), dtype=np.uint8)  # round-major: one contiguous array per call
    for r in range(K):
        host[:, r, :] = np.frombuffer(streams[r % 8], dtype=np.uint8).reshape(rounds, B)
    dev = torch.from_numpy(host).cuda()
    L = capi._group_lib()
    flags = capi.WIRE_VERBATIM if a.verbatim else 0
    res = {"receivers": K, "bytes_per_entry": B, "reps": a.reps, "wire_format": a.format, "verbatim": bool(a.verbatim),
           "calls_timed": "one msd_group_accept_beast, one msd_group_accept_beast_wire and one "
                          "msd_group_accept_beast_fields per round, no sink, on groups of their own, alternating in one process"}
    for where in ("device", "host"):
        groups = {"plain": capi.ReceiverGroup(K, fmt=capi.FMT_UC8), "wire": capi.ReceiverGroup(K, fmt=capi.FMT_UC8),
                  "fields": capi.ReceiverGroup(K, fmt=capi.FMT_UC8, flags=capi.CFG_DECODE_FIELDS)}
        ent = (capi.GroupBeastEntry * K)()
        t = {k: [] for k in groups}
        on_device = 1 if where == "device" else 0
        for k in range(rounds):
            base = k * K * B
            for i in range(K):
                ent[i] = capi.GroupBeastEntry(i, 0, base + i * B, B, 0, 1000 + k)
            ptr = C.c_void_p(dev.data_ptr() if on_device else host.ctypes.data)
            calls = {"plain": lambda h: L.msd_group_accept_beast(h, ptr, on_device, ent, K, None, None),
                     "wire": lambda h: L.msd_group_accept_beast_wire(h, ptr, on_device, ent, K, a.format, flags, None, None),
                     "fields": lambda h: L.msd_group_accept_beast_fields(h, ptr, on_device, ent, K, None, None)}
            for name, grp in groups.items():
                t0 = time.perf_counter()
                rc = calls[name](grp._h)
                t1 = time.perf_counter()
                assert rc == 0, (name, L.msd_group_last_error(grp._h))
                if k:  # (round 0 is the warm-up)
                    t[name].append(t1 - t0)
        row = {}
        for name in groups:
            row[name + "_call_ms_median"] = float(np.median(t[name])) * 1e3
            row[name + "_call_ms_all"] = [x * 1e3 for x in t[name]]
        for name in ("wire", "fields"):
            row[name + "_over_plain"] = row[name + "_call_ms_median"] / row["plain_call_ms_median"]
        for i in (0, K // 2, K - 1):  # the same bytes in the same calls: the same counters
            st = [grp.remote_stats(i) for grp in groups.values()]
            for s in st:
                s.pop("tile_rewalks")
            assert st[0] == st[1] == st[2], (i, st)
        row["counters_equal"] = True
        row["accepted_receiver_0"] = sum(groups["plain"].remote_stats(0)["remote_accepted"])
        res[where] = row
        print(where, json.dumps({k: round(v, 3) for k, v in row.items() if k.endswith("median") or k.endswith("plain")}),
              flush=True)
        for grp in groups.values():
            grp.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
