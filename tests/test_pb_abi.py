"""aircraft.pb's C-ABI (msd_pos_pb_enable, msd_pos_aircraft_pb; msd_pos_host_* in libmsd_host.so): declared, exported and
listed, msd_pb_options and msd_pb_receiver laid out as the Python mirrors say, MSD_PB_AIRCRAFT_MAX the sum of the field
maxima, every -EINVAL modes_hip.h names and the -ENOSPC / size / repeat rule -- on the host object here, on the device
object in a test marked gpu (a NULL tracker is refused by the device library without a device)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import pb_streams as pbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_pos_pb_enable", "msd_pos_aircraft_pb")


def test_declared_exported_and_listed(pkg):
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())
    assert "int msd_pos_pb_enable(msd_pos *p);" in hdr
    assert ("int msd_pos_aircraft_pb(msd_pos *p, const msd_pb_options *opt, uint8_t *out, size_t cap, size_t *out_len, "
            "msd_pb_receiver *rx);") in hdr
    assert "---- aircraft.pb:" in hdr
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    for n in NAMES:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
        assert hasattr(host, n.replace("msd_pos_", "msd_pos_host_"))


def test_struct_layouts_and_constants(pkg, tmp_path):
    names = {"msd_pb_options": ["now_ms", "messages_total", "flags", "reserved"],
             "msd_pb_receiver": ["end", "aircraft", "with_positions", "tisb_positions", "reserved"]}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
        f'printf("{s}.{m} %zu\\n", offsetof({s}, {m}));' for m in ms) for s, ms in names.items())
    body += 'printf("MSD_PB_AIRCRAFT_MAX %u\\n", (unsigned)MSD_PB_AIRCRAFT_MAX);'
    body += 'printf("MSD_PB_RSSI_MARGIN_ULPS %u\\n", (unsigned)MSD_PB_RSSI_MARGIN_ULPS);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_hip.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    capi = pkg.capi
    assert got["msd_pb_options"] == C.sizeof(capi.PbOptions) == 24
    for m in names["msd_pb_options"]:
        assert got[f"msd_pb_options.{m}"] == getattr(capi.PbOptions, m).offset, m
    assert got["msd_pb_receiver"] == capi.PB_RECEIVER_DTYPE.itemsize == 24
    for m in names["msd_pb_receiver"]:
        assert got[f"msd_pb_receiver.{m}"] == capi.PB_RECEIVER_DTYPE.fields[m][1], m
    assert got["MSD_PB_RSSI_MARGIN_ULPS"] == capi.PB_RSSI_MARGIN_ULPS == 8
    # the longest entry, field by field as the header's comment adds it up: tag bytes + value bytes
    body = [1 + 4, 1 + 1 + 8, 1 + 3, 1 + 2, 1 + 10, 1 + 3, 1 + 5, 1 + 8, 1 + 8, 1 + 10, 1 + 10, 1 + 4, 1 + 2]  # 1 .. 15
    body += [2 + 10] * 3 + [2 + 5] * 2 + [2 + 4, 2 + 3, 2 + 3] + [2 + 4] * 3 + [2 + 10] * 2 + [2 + 3]             # 20 .. 33
    body += [2 + 2, 2 + 3, 2 + 1] + [2 + 2] * 4 + [2 + 5, 2 + 1, 2 + 1, 2 + 2, 2 + 2] + [2 + 2] * 3               # 34 .. 102
    body += [2 + 1 + 6 * 2, 2 + 2 + 32 * (2 + 2)]                                                                # 150, 151
    assert sum(body) == 412 and 1 + 2 + sum(body) == got["MSD_PB_AIRCRAFT_MAX"] == capi.PB_AIRCRAFT_MAX == 415


def refusals(pkg, host):
    capi = pkg.capi

    def code(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code
    t = capi.PositionTracker(capacity=64, host=host)  # no table
    assert code(t.pb_enable) == -errno.EINVAL
    t.close()
    sc = pbs.TABLES["kinds"](pkg)
    t = capi.PositionTracker(capacity=64, host=host, table=True)
    t.update_nicrc(*sc[1][0][1:])
    assert code(lambda: t.aircraft_pb_stream(pbs.T0)) == -errno.EINVAL  # not enabled
    t.pb_enable()
    t.pb_enable()  # a second call changes nothing
    for bad in (dict(flags=1), dict(flags=1 << 31), dict(reserved=1)):
        assert code(lambda: t.aircraft_pb_stream(pbs.T0, **bad)) == -errno.EINVAL, bad
    fn, tail = t.f["aircraft_pb"], ([None] if host else [])
    opt, need = capi.PbOptions(now_ms=pbs.T0 + 2000), C.c_size_t(7)
    out = np.zeros(4096, dtype=np.uint8)
    rx = np.zeros(1, dtype=capi.PB_RECEIVER_DTYPE)
    assert fn(None, C.byref(opt), out.ctypes.data, 4096, C.byref(need), rx.ctypes.data, *tail) == -errno.EINVAL
    assert fn(t.h, None, out.ctypes.data, 4096, C.byref(need), rx.ctypes.data, *tail) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), out.ctypes.data, 4096, None, rx.ctypes.data, *tail) == -errno.EINVAL
    assert fn(t.h, C.byref(opt), None, 4096, C.byref(need), rx.ctypes.data, *tail) == -errno.EINVAL
    # the size: -ENOSPC with nothing written, as often as asked; then the bytes the first call would have given
    out[:] = 0xEE
    rx["end"] = 77
    for cap in (0, 1, 100):
        assert fn(t.h, C.byref(opt), out.ctypes.data, cap, C.byref(need), rx.ctypes.data, *tail) == -errno.ENOSPC
        assert need.value > 800 and (out == 0xEE).all() and int(rx["end"][0]) == 77
    size = need.value
    assert fn(t.h, C.byref(opt), out.ctypes.data, size, C.byref(need), None, *tail) == 0 and need.value == size  # rx may be NULL
    first = out[:size].tobytes()
    assert (out[size:] == 0xEE).all()
    fresh = capi.PositionTracker(capacity=64, host=host, table=True, pb=True)
    fresh.update_nicrc(*sc[1][0][1:])
    stream, rows = fresh.aircraft_pb_stream(pbs.T0 + 2000)
    assert stream == first and int(rows["end"][0]) == size and int(rows["aircraft"][0]) == 18
    t.close(), fresh.close()


def test_refusals_on_the_host_object(pkg):
    refusals(pkg, True)


def test_null_tracker_is_refused_by_the_device_library(pkg):
    lib = pkg.capi.lib()
    assert lib.msd_pos_pb_enable(None) == -errno.EINVAL
    assert lib.msd_pos_aircraft_pb(None, None, None, 0, None, None) == -errno.EINVAL


@pytest.mark.gpu
def test_refusals_on_the_device_object(pkg, torch_cuda):
    refusals(pkg, False)
