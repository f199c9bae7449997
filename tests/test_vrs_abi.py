"""The VRS output's C-ABI (msd_pos_vrs_enable, msd_pos_vrs; msd_pos_host_* in libmsd_host.so): declared, exported and
listed, msd_vrs_options and msd_vrs_receiver laid out as the Python mirrors say, MSD_VRS_AIRCRAFT_MAX the sum of its
terms and reached exactly by one constructed aircraft, every -EINVAL modes_hip.h names and the -ENOSPC / size / repeat
rule on the host object (on the device object: test_gpu_vrs.py; a NULL tracker is refused by the device library without a
device)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import vrs_streams as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_pos_vrs_enable", "msd_pos_vrs")
# the longest object, key by key as the header's comment adds it up: the key with its punctuation + the widest value
TERMS = [1,                  # the comma
         len('{"Sig":') + 10, len(',"Icao":"') + 6 + 1, len(',"Alt":') + 11, len(',"GAlt":') + 11, len(',"InHg":') + 7,
         len(',"TAlt":') + 11, len(',"Call":"') + 8 * 6 + 1, len(',"Lat":') + 11, len(',"Long":') + 11,
         len(',"PosTime":') + 20, len(',"Mlat":') + 5, len(',"Tisb":') + 5, len(',"Spd":') + 11, len(',"SpdTyp":') + 1,
         len(',"Trak":') + 6, len(',"TrkH":') + 5, len(',"TTrk":') + 5, len(',"Sqk":"') + 4 + 1, len(',"Vsi":') + 11,
         len(',"VsiT":') + 1, len(',"Gnd":') + 5, len(',"Trt":') + 3, len(',"Cmsgs":') + 20, 1]


def test_declared_exported_and_listed(pkg):
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())
    assert "int msd_pos_vrs_enable(msd_pos *p);" in hdr
    assert ("int msd_pos_vrs(msd_pos *p, const msd_vrs_options *opt, uint8_t *out, size_t cap, size_t *out_len, "
            "msd_vrs_receiver *rx);") in hdr
    assert "---- VRS output:" in hdr
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    for n in NAMES:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
        assert hasattr(host, n.replace("msd_pos_", "msd_pos_host_"))


def test_struct_layouts_and_constants(pkg, tmp_path):
    names = {"msd_vrs_options": ["now_ms", "part", "n_parts", "flags", "reserved"],
             "msd_vrs_receiver": ["end", "aircraft", "reserved"]}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
        f'printf("{s}.{m} %zu\\n", offsetof({s}, {m}));' for m in ms) for s, ms in names.items())
    body += 'printf("MSD_VRS_AIRCRAFT_MAX %u\\n", (unsigned)MSD_VRS_AIRCRAFT_MAX);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_hip.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    capi = pkg.capi
    assert got["msd_vrs_options"] == C.sizeof(capi.VrsOptions) == 24
    for m in names["msd_vrs_options"]:
        assert got[f"msd_vrs_options.{m}"] == getattr(capi.VrsOptions, m).offset, m
    assert got["msd_vrs_receiver"] == capi.VRS_RECEIVER_DTYPE.itemsize == 16  # no implicit padding: 8 + 4 + 4
    for m in names["msd_vrs_receiver"]:
        assert got[f"msd_vrs_receiver.{m}"] == capi.VRS_RECEIVER_DTYPE.fields[m][1], m
    assert sum(TERMS) == got["MSD_VRS_AIRCRAFT_MAX"] == capi.VRS_AIRCRAFT_MAX == 418


def test_the_tables_tile_is_the_kernels(pkg):
    src = open(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_pos.h")).read()
    assert int(re.search(r"#define MSD_VRS_TILE (\d+)u", src).group(1)) == vs.TILE


def test_one_constructed_aircraft_reaches_the_maximum(pkg):
    """every key present and every value at its widest, written by the host object's writer of one entry"""
    capi = pkg.capi
    L, _ = capi._pos_lib(True)
    now = 1_700_000_000_000
    e = np.zeros((), dtype=capi.AIRCRAFT_DTYPE)
    e["source"][:] = 7
    e["updated"][:] = now
    e["updated"][capi.AC["position"]] = (1 << 64) - 1 - 70000  # twenty digits, and updated + 70 s does not wrap
    e["altitude_geom_expires"] = now + 1
    e["signal_level"][:] = 1.5e7                               # Sig 3825000000
    e["addr"], e["altitude_baro_reliable"], e["messages"] = 0xFFFFFF, 3, (1 << 64) - 1
    for k in ("alt_baro", "alt_geom", "nav_altitude_mcp", "geom_rate"):
        e[k] = -(1 << 31)
    e["nav_qnh_raw"], e["nav_heading_raw"], e["squawk"], e["adsb_version"] = 65535, 65535, 0xFFFF, 127
    e["callsign"] = b"\xff" * 8
    e["lat"] = e["lon"] = -360.0
    e["gs"] = 1 << 31                                          # %d of a uint32_t: -2147483648
    e["track"]["kind"], e["track"]["raw"] = 3, 65535           # MSD_HDG_SURFACE: 65535 x 360 / 128 = 184317
    out = C.create_string_buffer(capi.VRS_AIRCRAFT_MAX + 2)
    n = L.msd_pos_host_vrs_object(e.ctypes.data, now, 1, out)
    assert n == capi.VRS_AIRCRAFT_MAX, (n, out.value)
    want = (',{"Sig":3825000000,"Icao":"FFFFFF","Alt":-2147483648,"GAlt":-2147483648,"InHg":1571.80,"TAlt":-2147483648,'
            '"Call":"' + "\\u00ff" * 8 + '","Lat":-360.000000,"Long":-360.000000,"PosTime":18446744073709481615,'
            '"Mlat":false,"Tisb":false,"Spd":-2147483648,"SpdTyp":0,"Trak":184317,"TrkH":false,"TTrk":65535,"Sqk":"ffff",'
            '"Vsi":-2147483648,"VsiT":1,"Gnd":false,"Trt":130,"Cmsgs":18446744073709551615}')
    assert out.value.decode() == want and len(want) == 418
    assert L.msd_pos_host_vrs_object(e.ctypes.data, now, 0, out) == capi.VRS_AIRCRAFT_MAX - 1


def test_refusals_on_the_host_object(pkg):
    capi = pkg.capi

    def code(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code
    t = capi.PositionTracker(capacity=64, host=True)  # no table
    assert code(t.vrs_enable) == -errno.EINVAL
    t.close()
    sc = vs.TABLES["kinds"](pkg)
    t = capi.PositionTracker(capacity=64, host=True, table=True)
    vs.run(t, (sc[0], sc[1], []))
    assert code(lambda: t.vrs_stream(vs.T0 + 2000)) == -errno.EINVAL  # not enabled
    t.vrs_enable()
    t.vrs_enable()  # a second call changes nothing
    for bad in (dict(flags=1), dict(flags=1 << 31), dict(reserved=1), dict(n_parts=0), dict(n_parts=3), dict(n_parts=4096),
                dict(n_parts=6), dict(part=1), dict(part=8, n_parts=8), dict(part=2048, n_parts=2048)):
        assert code(lambda: t.vrs_stream(vs.T0 + 2000, **bad)) == -errno.EINVAL, bad
    fn = t.f["vrs"]
    opt, need = capi.VrsOptions(now_ms=vs.T0 + 2000, part=0, n_parts=1), C.c_size_t(7)
    out = np.zeros(8192, dtype=np.uint8)
    rx = np.zeros(1, dtype=capi.VRS_RECEIVER_DTYPE)
    assert fn(None, C.byref(opt), out.ctypes.data, 8192, C.byref(need), rx.ctypes.data) == -errno.EINVAL
    assert fn(t.h, None, out.ctypes.data, 8192, C.byref(need), rx.ctypes.data) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), out.ctypes.data, 8192, None, rx.ctypes.data) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), None, 8192, C.byref(need), rx.ctypes.data) == -errno.EINVAL
    # the size: -ENOSPC with nothing written, as often as asked; then the bytes, the same on every call
    out[:] = 0xEE
    rx["end"] = 77
    for cap in (0, 1, 100):
        assert fn(t.h, C.byref(opt), out.ctypes.data, cap, C.byref(need), rx.ctypes.data) == -errno.ENOSPC
        assert need.value > 2000 and (out == 0xEE).all() and int(rx["end"][0]) == 77
    size = need.value
    assert fn(t.h, C.byref(opt), out.ctypes.data, size, C.byref(need), None) == 0 and need.value == size  # rx may be NULL
    first = out[:size].tobytes()
    assert (out[size:] == 0xEE).all()
    stream, rows = t.vrs_stream(vs.T0 + 2000)
    assert stream == first and int(rows["end"][0]) == size and int(rows["aircraft"][0]) == 28
    t.close()


def test_null_tracker_is_refused_by_the_device_library(pkg):
    lib = pkg.capi.lib()
    assert lib.msd_pos_vrs_enable(None) == -errno.EINVAL
    assert lib.msd_pos_vrs(None, None, None, 0, None, None) == -errno.EINVAL
