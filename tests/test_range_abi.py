"""The receiver range's C-ABI (msd_pos_range_enable / _read / _distances / _margins; msd_pos_host_range_* in
libmsd_host.so): declared, exported and listed, msd_range_receiver and msd_range_margins laid out as the Python mirrors say,
the constants, and every refusal modes_hip.h names -- on the host object here (the device object's are in
tests/test_gpu_range.py; a NULL tracker is refused by the device library without a device)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import range_streams as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_pos_range_enable", "msd_pos_range_read", "msd_pos_range_distances", "msd_pos_range_margins", "msd_pos_range_pb")


def test_declared_exported_and_listed(pkg):
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())
    assert "int msd_pos_range_enable(msd_pos *p, uint32_t flags);" in hdr
    assert "int msd_pos_range_read(msd_pos *p, uint32_t first, uint32_t count, msd_range_receiver *out, uint32_t flags);" in hdr
    assert "int msd_pos_range_distances(msd_pos *p, uint32_t *out, size_t cap, int on_device, size_t *n);" in hdr
    assert "int msd_pos_range_margins(const msd_pos *p, msd_range_margins *m);" in hdr
    assert "int msd_pos_range_pb(msd_pos *p, uint8_t *out, size_t cap, size_t *out_len, uint64_t *end);" in hdr
    assert "---- Receiver range:" in hdr
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    for n in NAMES:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
        assert hasattr(host, n.replace("msd_pos_", "msd_pos_host_"))


def test_struct_layouts_and_constants(pkg, tmp_path):
    names = {"msd_range_receiver": ["polar_range", "longest_m", "longest_nm", "evaluated"],
             "msd_range_margins": ["min_range_margin_m", "min_bearing_margin_deg"]}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
        f'printf("{s}.{m} %zu\\n", offsetof({s}, {m}));' for m in ms) for s, ms in names.items())
    for k in ("MSD_RANGE_BUCKETS", "MSD_RANGE_POLAR", "MSD_RANGE_TAKE_LONGEST", "MSD_PB_AIRCRAFT_MAX", "MSD_PB_AIRCRAFT_MAX_RANGE",
              "MSD_RANGE_PB_ENTRY_MAX"):
        body += f'printf("{k} %u\\n", (unsigned){k});'
    body += 'printf("MARGIN_NM %.0f\\n", MSD_RANGE_MARGIN_M * 1e9); printf("MARGIN_NDEG %.0f\\n", MSD_RANGE_BEARING_MARGIN_DEG * 1e9);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_hip.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    capi = pkg.capi
    assert got["msd_range_receiver"] == capi.RANGE_RECEIVER_DTYPE.itemsize == 304 == 4 * 72 + 4 + 4 + 8  # no padding
    for m in names["msd_range_receiver"]:
        assert got[f"msd_range_receiver.{m}"] == capi.RANGE_RECEIVER_DTYPE.fields[m][1], m
    assert got["msd_range_margins"] == C.sizeof(capi.RangeMargins) == 16
    for m in names["msd_range_margins"]:
        assert got[f"msd_range_margins.{m}"] == getattr(capi.RangeMargins, m).offset, m
    assert got["MSD_RANGE_BUCKETS"] == capi.RANGE_BUCKETS == 72 and 72 * 5 == 360
    assert got["MSD_RANGE_POLAR"] == capi.RANGE_POLAR == 1 and got["MSD_RANGE_TAKE_LONGEST"] == capi.RANGE_TAKE_LONGEST == 1
    assert got["MARGIN_NM"] == round(capi.RANGE_MARGIN_M * 1e9) == 10 ** 6
    assert got["MARGIN_NDEG"] == round(capi.RANGE_BEARING_MARGIN_DEG * 1e9) == 10 ** 4
    # the two *_MAX figures are the sums of their terms: the entry of a tracker without the range, the tag 0x68 (13 << 3) and a
    # uint32's longest varint; the tag 0x32 and a length, 08 and the bucket (below 128), 10 and a uint32's longest varint
    assert got["MSD_PB_AIRCRAFT_MAX_RANGE"] == capi.PB_AIRCRAFT_MAX_RANGE == got["MSD_PB_AIRCRAFT_MAX"] + 1 + 5 == 421
    assert 13 << 3 == 0x68 and len(rs.ir.varint(0xFFFFFFFF)) == 5 and len(rs.ir.varint(71)) == 1
    assert got["MSD_RANGE_PB_ENTRY_MAX"] == capi.RANGE_PB_ENTRY_MAX == (1 + 1) + (1 + 1) + (1 + 5) == 10
    assert len(rs.ir.polar_range_pb([0xFFFFFFFF] * 72)) == 8 + 71 * 10
    # the streams of the tests keep fifty and a thousand times the contract
    assert rs.RANGE_MARGIN == 50 * capi.RANGE_MARGIN_M and rs.BEARING_MARGIN == 1000 * capi.RANGE_BEARING_MARGIN_DEG


def code_of(pkg, call):
    with pytest.raises(pkg.MsdError) as e:
        call()
    return e.value.code


def test_refusals_on_the_host_object(pkg):
    capi = pkg.capi
    t = capi.PositionTracker(capacity=64, host=True)
    for call in (t.range_read, t.range_distances, t.range_margins):
        assert code_of(pkg, call) == -errno.EINVAL  # not enabled
    for flags in (2, 3, 1 << 31):
        assert code_of(pkg, lambda: t.range_enable(flags)) == -errno.EINVAL
    t.range_enable(capi.RANGE_POLAR)
    t.range_enable(0)  # a second call returns 0 and changes nothing
    row = np.zeros(1, dtype=capi.RANGE_RECEIVER_DTYPE)
    n = C.c_size_t(9)
    assert t.f["range_read"](None, 0, 1, row.ctypes.data, 0) == -errno.EINVAL
    assert t.f["range_read"](t.h, 0, 1, None, 0) == -errno.EINVAL
    assert t.f["range_read"](t.h, 0, 2, row.ctypes.data, 0) == -errno.EINVAL
    assert t.f["range_read"](t.h, 1, 1, row.ctypes.data, 0) == -errno.EINVAL
    assert t.f["range_read"](t.h, 0, 1, row.ctypes.data, 2) == -errno.EINVAL
    assert t.f["range_read"](t.h, 1, 0, None, 0) == 0
    assert t.f["range_distances"](None, None, 0, C.byref(n)) == -errno.EINVAL
    assert t.f["range_distances"](t.h, None, 0, None) == -errno.EINVAL
    assert t.f["range_distances"](t.h, None, 0, C.byref(n)) == 0 and n.value == 0  # no aircraft
    assert t.f["range_margins"](t.h, None) == -errno.EINVAL and t.f["range_margins"](None, None) == -errno.EINVAL
    out = np.full(512, 0xEE, dtype=np.uint8)
    end = np.full(1, 77, dtype=np.uint64)
    assert t.f["range_pb"](None, out.ctypes.data, 512, C.byref(n), end.ctypes.data) == -errno.EINVAL
    assert t.f["range_pb"](t.h, None, 512, C.byref(n), end.ctypes.data) == -errno.EINVAL
    assert t.f["range_pb"](t.h, out.ctypes.data, 512, None, end.ctypes.data) == -errno.EINVAL
    for cap in (0, 285):  # -ENOSPC: the size, and nothing written
        assert t.f["range_pb"](t.h, out.ctypes.data, cap, C.byref(n), end.ctypes.data) == -errno.ENOSPC
        assert n.value == 286 and (out == 0xEE).all() and int(end[0]) == 77
    assert t.f["range_pb"](t.h, out.ctypes.data, 286, C.byref(n), None) == 0 and n.value == 286 and (out[286:] == 0xEE).all()
    assert out[:6].tobytes() == bytes.fromhex("320032020801")
    t.close()
    t = capi.PositionTracker(capacity=64, host=True, range=True, polar=False)
    assert code_of(pkg, t.range_pb) == -errno.EINVAL  # enabled without MSD_RANGE_POLAR
    t.close()


def test_null_tracker_is_refused_by_the_device_library(pkg):
    lib = pkg.capi.lib()
    assert lib.msd_pos_range_enable(None, 0) == -errno.EINVAL
    assert lib.msd_pos_range_read(None, 0, 0, None, 0) == -errno.EINVAL
    assert lib.msd_pos_range_distances(None, None, 0, 0, None) == -errno.EINVAL
    assert lib.msd_pos_range_margins(None, None) == -errno.EINVAL
    assert lib.msd_pos_range_pb(None, None, 0, None, None) == -errno.EINVAL
