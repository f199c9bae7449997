"""The C-ABI of history_N.pb and receiver.pb (msd_pos_history_pb, msd_receiver_pb; msd_pos_host_history_pb in
libmsd_host.so): declared, exported and listed, the structs laid out as the Python mirrors say, MSD_HISTORY_ENTRY_MAX the
sum of its terms and reached exactly by one constructed entry, and a NULL tracker refused without a device."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np

import indep_history as ih

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = [1, 1,       # the tag 0x72 and a one-byte length
         1 + 4,      # addr: 25 bits are a four-byte varint
         1 + 10,     # alt_baro: a negative int32 is sign-extended
         1 + 8, 1 + 8]


def test_declared_exported_and_listed(pkg):
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())
    assert ("int msd_pos_history_pb(msd_pos *p, const msd_history_options *opt, uint8_t *out, size_t cap, size_t *out_len, "
            "msd_history_receiver *rx);") in hdr
    assert "int msd_receiver_pb(const msd_receiver_info *info, uint8_t *out, size_t cap, size_t *out_len);" in hdr
    assert hdr.index("---- VRS output:") < hdr.index("---- history_N.pb:") < hdr.index("---- Receiver range:")
    twin = re.sub(r"\s+", " ", open(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "host", "msd_pos_host.h")).read())
    assert "int msd_pos_host_history_pb(msd_pos_host *p, const msd_history_options *opt," in twin
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    for n in ("msd_pos_history_pb", "msd_receiver_pb"):
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
    assert hasattr(host, "msd_pos_host_history_pb") and hasattr(host, "msd_pos_host_history_entry")
    assert hasattr(host, "msd_receiver_pb")  # the one host file is in both libraries


def test_struct_layouts_and_constants(pkg, tmp_path):
    names = {"msd_history_options": ["now_ms", "flags", "reserved"],
             "msd_history_receiver": ["end", "aircraft", "reserved"],
             "msd_receiver_info": ["version", "latitude", "longitude", "refresh", "altitude", "antenna_serial", "antenna_flags",
                                   "antenna_gps_sats", "antenna_gps_hdop", "antenna_reserved", "history", "location_accuracy",
                                   "reserved"]}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
        f'printf("{s}.{m} %zu\\n", offsetof({s}, {m}));' for m in ms) for s, ms in names.items())
    body += 'printf("MSD_HISTORY_ENTRY_MAX %u\\n", (unsigned)MSD_HISTORY_ENTRY_MAX);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_hip.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    capi = pkg.capi
    assert got["msd_history_options"] == C.sizeof(capi.HistoryOptions) == 16
    assert got["msd_history_receiver"] == C.sizeof(capi.HistoryReceiver) == capi.HISTORY_RECEIVER_DTYPE.itemsize == 16
    assert got["msd_receiver_info"] == C.sizeof(capi.ReceiverInfo) == 64
    for s, mirror in (("msd_history_options", capi.HistoryOptions), ("msd_history_receiver", capi.HistoryReceiver),
                      ("msd_receiver_info", capi.ReceiverInfo)):
        assert [m for m, _ in mirror._fields_] == names[s]
        for m in names[s]:
            assert got[f"{s}.{m}"] == getattr(mirror, m).offset, (s, m)
    for m in names["msd_history_receiver"]:
        assert got[f"msd_history_receiver.{m}"] == capi.HISTORY_RECEIVER_DTYPE.fields[m][1], m
    assert sum(TERMS) == got["MSD_HISTORY_ENTRY_MAX"] == capi.HISTORY_ENTRY_MAX == 36


def test_one_constructed_entry_reaches_the_maximum(pkg):
    """the non-ICAO address bit set, a negative altitude, both coordinates non-zero"""
    capi = pkg.capi
    L, _ = capi._pos_lib(True)
    now = 1_700_000_000_000
    e = np.zeros((), dtype=capi.AIRCRAFT_DTYPE)
    e["addr"] = (1 << 24) | 0x4840D6
    e["source"][capi.AC["altitude_baro"]], e["updated"][capi.AC["altitude_baro"]] = 7, now
    e["altitude_baro_reliable"], e["alt_baro"] = 3, -1
    e["lat"], e["lon"] = -89.5, 179.5
    out = np.full(capi.HISTORY_ENTRY_MAX + 1, 0xEE, dtype=np.uint8)
    n = L.msd_pos_host_history_entry(e.ctypes.data, now, out.ctypes.data)
    assert n == capi.HISTORY_ENTRY_MAX and out[n] == 0xEE
    got = out[:n].tobytes()
    assert got[:2] == b"\x72\x22" and got == ih.entry(e, capi.AC, now)
    assert ih.read_file(got)["history"] == [dict(addr=(1 << 24) | 0x4840D6, alt_baro=-1, lat=-89.5, lon=179.5)]
    e["addr"] = 0x1FFFFFF  # every stored bit: still four bytes
    assert L.msd_pos_host_history_entry(e.ctypes.data, now, None) == capi.HISTORY_ENTRY_MAX


def test_null_tracker_is_refused_by_the_device_library(pkg):
    lib = pkg.capi.lib()
    assert lib.msd_pos_history_pb(None, None, None, 0, None, None) == -errno.EINVAL
