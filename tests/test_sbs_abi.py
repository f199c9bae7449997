"""The SBS output's C-ABI (msd_pos_sbs_enable, msd_pos_update_sbs, msd_pos_sbs_wire; msd_pos_host_* in libmsd_host.so):
declared, exported and listed, msd_sbs_track and msd_sbs_options laid out as the Python mirrors say, MSD_SBS_MAX the sum
of the field maxima, and -EINVAL for every refusal modes_hip.h names -- on the host twin here, on the device object in a
test marked gpu (a NULL tracker is refused by the device library without a device)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import sbs_streams as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_pos_sbs_enable", "msd_pos_update_sbs", "msd_pos_sbs_wire")
YEAR_10000 = 253402300800000


def test_declared_exported_and_listed(pkg):
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())
    assert "int msd_pos_sbs_enable(msd_pos *p);" in hdr
    assert ("int msd_pos_update_sbs(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, "
            "size_t n, int on_device, msd_position *out, msd_pos_nicrc *nicrc, uint8_t *forward, msd_sbs_track *trk);") in hdr
    assert ("int msd_pos_sbs_wire(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk, "
            "size_t n, int on_device, const msd_sbs_options *opt, uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends);") in hdr
    assert "---- SBS output:" in hdr
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    for n in NAMES:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
        assert hasattr(host, n.replace("msd_pos_", "msd_pos_host_"))


def test_struct_layouts_and_constants(pkg, tmp_path):
    names = {"msd_sbs_track": ["lat", "lon", "gs_selected", "geom_delta", "flags", "pad"],
             "msd_sbs_options": ["now_ms", "utc_offset_ms", "flags", "reserved"]}
    consts = ["MSD_SBS_TRACKED", "MSD_SBS_SEEN_TWICE", "MSD_SBS_GS_VALID", "MSD_SBS_GEOM_DELTA_VALID", "MSD_SBS_CPR_DECODED",
              "MSD_SBS_NET_ONLY", "MSD_SBS_GNSS", "MSD_SBS_NOW_IS_RECEIVED", "MSD_SBS_MAX", "MSD_WIRE_VERBATIM"]
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
        f'printf("{s}.{m} %zu\\n", offsetof({s}, {m}));' for m in ms) for s, ms in names.items())
    body += "".join(f'printf("{c} %u\\n", (unsigned){c});' for c in consts)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_hip.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    capi = pkg.capi
    assert got["msd_sbs_track"] == capi.SBS_TRACK_DTYPE.itemsize == 32
    for m in names["msd_sbs_track"]:
        assert got[f"msd_sbs_track.{m}"] == capi.SBS_TRACK_DTYPE.fields[m][1], m
    assert sum(capi.SBS_TRACK_DTYPE.fields[m][0].itemsize for m in names["msd_sbs_track"]) == 32  # no implicit padding
    assert got["msd_sbs_options"] == C.sizeof(capi.SbsOptions) == 24
    for m in names["msd_sbs_options"]:
        assert got[f"msd_sbs_options.{m}"] == getattr(capi.SbsOptions, m).offset, m
    assert [got[c] for c in consts] == [capi.SBS_TRACKED, capi.SBS_SEEN_TWICE, capi.SBS_GS_VALID, capi.SBS_GEOM_DELTA_VALID,
                                        capi.SBS_CPR_DECODED, capi.SBS_NET_ONLY, capi.SBS_GNSS, capi.SBS_NOW_IS_RECEIVED,
                                        capi.SBS_MAX, capi.WIRE_VERBATIM]
    # the longest line, field by field as the header's comment adds them up; prepareWrite asks for 200
    parts = ["MSG,1,1,1,FFFFFF,1,", "YYYY/MM/DD,HH:MM:SS.mmm,", "YYYY/MM/DD,HH:MM:SS.mmm", ",WWWWWWWW", ",-2147483648H", ",65535",
             ",360", ",-180.00000,-180.00000", ",-32768H", ",7700", ",-1", ",-1", ",-1", ",-1", "\r\n"]
    assert sum(len(x) for x in parts) == got["MSD_SBS_MAX"] == 147 <= 200


def refusals(pkg, host):
    """every -EINVAL of the three calls on one library"""
    capi = pkg.capi
    s = ss.scenarios(pkg)["delivery"]
    m, f, r = ss.records(s["steps"])

    def code(call):
        with pytest.raises(pkg.MsdError) as e:
            call()
        return e.value.code
    t = capi.PositionTracker(capacity=64, host=host)  # no table
    assert code(t.sbs_enable) == -errno.EINVAL
    t.close()
    t = capi.PositionTracker(capacity=64, host=host, table=True)  # not enabled
    trk = np.zeros(len(m), dtype=capi.SBS_TRACK_DTYPE)
    assert code(lambda: t.update_sbs(m, f, r)) == -errno.EINVAL
    assert code(lambda: t.sbs_wire(m, f, trk)) == -errno.EINVAL
    t.sbs_enable()
    t.sbs_enable()  # a second call changes nothing
    assert code(lambda: t.update_sbs(m, f, r, forward=True)) == -errno.EINVAL  # verdicts need a tracker that reduces
    trk = t.update_sbs(m, f, r)[3]
    assert len(t.sbs_wire(m, f, trk, now_ms=ss.T0)[0]) > 0
    for bad in (dict(flags=16), dict(flags=1 << 31), dict(reserved=1), dict(now_ms=0, utc_offset_ms=-1),
                dict(now_ms=YEAR_10000), dict(now_ms=YEAR_10000 - 1, utc_offset_ms=1), dict(now_ms=(1 << 64) - 1, utc_offset_ms=1),
                dict(now_ms=5, utc_offset_ms=-(1 << 63)), dict(now_ms=0, utc_offset_ms=-1, now_is_received=True)):
        assert code(lambda: t.sbs_wire(m, f, trk, **bad)) == -errno.EINVAL, bad
    for good in (dict(now_ms=YEAR_10000 - 1), dict(now_ms=YEAR_10000, utc_offset_ms=-1), dict(now_ms=1, utc_offset_ms=-1)):
        t.sbs_wire(m, f, trk, **good)
    fn, dev = t.f["sbs_wire"], ([] if host else [0])
    opt, need = capi.SbsOptions(now_ms=ss.T0), C.c_size_t(7)
    out = np.zeros(4096, dtype=np.uint8)
    args = (m.ctypes.data, f.ctypes.data, trk.ctypes.data)
    assert fn(t.h, None, None, None, 0, *dev, C.byref(opt), None, 0, C.byref(need), None) == 0 and need.value == 0
    assert fn(None, *args, len(m), *dev, C.byref(opt), out.ctypes.data, 4096, C.byref(need), None) == -errno.EINVAL
    assert fn(t.h, *args, len(m), *dev, None, out.ctypes.data, 4096, C.byref(need), None) == -errno.EINVAL
    assert fn(t.h, *args, len(m), *dev, C.byref(opt), out.ctypes.data, 4096, None, None) == -errno.EINVAL
    assert fn(t.h, *args, len(m), *dev, C.byref(opt), None, 4096, C.byref(need), None) == -errno.EINVAL
    assert fn(t.h, *args, (1 << 24) + 1, *dev, C.byref(opt), out.ctypes.data, 4096, C.byref(need), None) == -errno.EINVAL
    for k in range(3):
        holed = list(args)
        holed[k] = None
        assert fn(t.h, *holed, len(m), *dev, C.byref(opt), out.ctypes.data, 4096, C.byref(need), None) == -errno.EINVAL
    up = t.f["update_sbs"]
    pos = np.zeros(len(m), dtype=capi.POSITION_DTYPE)
    assert up(t.h, m.ctypes.data, f.ctypes.data, None, len(m), *dev, pos.ctypes.data, None, None, None) == -errno.EINVAL
    assert up(None, m.ctypes.data, f.ctypes.data, None, len(m), *dev, pos.ctypes.data, None, None, trk.ctypes.data) == -errno.EINVAL
    assert up(t.h, None, None, None, 0, *dev, None, None, None, None) == 0
    t.close()


def test_refusals_on_the_twin(pkg):
    refusals(pkg, True)


def test_null_tracker_is_refused_by_the_device_library(pkg):
    lib = pkg.capi.lib()
    assert lib.msd_pos_sbs_enable(None) == -errno.EINVAL


@pytest.mark.gpu
def test_refusals_on_the_device_object(pkg, torch_cuda):
    refusals(pkg, False)
