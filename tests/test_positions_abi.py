"""The position tracker's C-ABI (msd_pos_*; msd_pos_host_* in libmsd_host.so): declared in modes_hip.h, exported,
listed in capi.EXPORTS, the structures laid out as the Python mirrors say, -EINVAL for NULL and for a receiver index out
of range, n == 0 (no GPU needed: the device object's argument checks come before it asks for a device, the rest runs on
the host twin)."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import pos_streams as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msd_pos_create", "msd_pos_destroy", "msd_pos_last_error", "msd_pos_reset", "msd_pos_set_receiver",
         "msd_pos_update", "msd_pos_expire", "msd_pos_get_stats")


def test_declared_exported_and_listed(pkg):
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "modes_hip.h")).read())
    assert ("int msd_pos_update(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, "
            "size_t n, int on_device, msd_position *out);") in hdr
    assert "int msd_pos_expire(msd_pos *p, uint64_t now_ms);" in hdr
    assert "1e-3 m" in hdr and "min_gate_margin_m" in hdr  # the gate-margin contract is written down
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    for n in NAMES:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
    for n in ("create", "destroy", "reset", "set_receiver", "update", "expire", "get_stats", "home_slot"):
        assert hasattr(host, "msd_pos_host_" + n)
    for n in ("airborne", "surface", "relative"):
        assert hasattr(host, "msd_cpr_host_" + n)


def test_struct_sizes_and_offsets(pkg, tmp_path):
    """The compiler's layout of the four structures against the ctypes / numpy mirrors."""
    src = tmp_path / "layout.c"
    names = {"msd_pos_receiver": ["lat", "lon", "max_range_m", "latlon_valid", "reserved"],
             "msd_pos_config": ["device", "filter_persistence", "capacity", "receivers", "receiver"],
             "msd_position": ["lat", "lon", "decoded", "relative", "surface", "result", "pad"],
             "msd_pos_stats": ["cpr_surface", "cpr_global_ok", "cpr_local_ok", "cpr_local_speed_checks", "aircraft",
                               "min_gate_margin_m"]}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
        f'printf("{s}.{m} %zu\\n", offsetof({s}, {m}));' for m in ms) for s, ms in names.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_hip.h"\nint main(void){' + body + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    capi = pkg.capi
    mirrors = {"msd_pos_receiver": capi.PosReceiver, "msd_pos_config": capi.PosConfig, "msd_pos_stats": capi.PosStats}
    for s, cls in mirrors.items():
        assert int(got[s]) == C.sizeof(cls)
        for m in names[s]:
            assert int(got[f"{s}.{m}"]) == getattr(cls, m).offset, (s, m)
    assert int(got["msd_position"]) == capi.POSITION_DTYPE.itemsize == 24
    for m in names["msd_position"]:
        assert int(got[f"msd_position.{m}"]) == capi.POSITION_DTYPE.fields[m][1]
    assert (int(got["msd_pos_receiver"]), int(got["msd_pos_config"]), int(got["msd_pos_stats"])) == (32, 24, 120)


def test_einval_for_null_and_bad_configurations(pkg):
    lib = pkg.capi.lib()
    host = C.CDLL(pkg.capi.HOST_LIB_PATH)
    h = C.c_void_p()
    st = pkg.capi.PosStats()
    good = dict(device=0, filter_persistence=0, capacity=64, receivers=1, receiver=None)
    for create in (lib.msd_pos_create, host.msd_pos_host_create):
        create.argtypes = [C.c_void_p, C.c_void_p]
        assert create(None, C.byref(h)) == -errno.EINVAL
        assert create(C.byref(pkg.capi.PosConfig(**good)), None) == -errno.EINVAL
        for bad in (dict(capacity=0), dict(capacity=63), dict(capacity=96), dict(capacity=1 << 25), dict(receivers=0),
                    dict(receivers=65537), dict(filter_persistence=-1)):
            assert create(C.byref(pkg.capi.PosConfig(**dict(good, **bad))), C.byref(h)) == -errno.EINVAL, bad
    for pre, L in (("msd_pos_", lib), ("msd_pos_host_", host)):
        assert getattr(L, pre + "reset")(None) == -errno.EINVAL
        assert getattr(L, pre + "expire")(None, C.c_uint64(0)) == -errno.EINVAL
        assert getattr(L, pre + "get_stats")(None, C.byref(st)) == -errno.EINVAL
        assert getattr(L, pre + "set_receiver")(None, 0, None) == -errno.EINVAL
        getattr(L, pre + "destroy")(None)
    lib.msd_pos_update.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_int, C.c_void_p]
    assert lib.msd_pos_update(None, None, None, None, 0, 0, None) == -errno.EINVAL
    lib.msd_pos_last_error.restype = C.c_char_p
    assert lib.msd_pos_last_error(None)


def test_no_cpu_fallback_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        return  # with a GPU the object exists: tests/test_gpu_positions.py
    with pytest.raises(pkg.MsdError) as e:
        pkg.capi.PositionTracker(capacity=64)
    assert str(-errno.ENODEV) in str(e.value)


def test_twin_argument_checks(pkg):
    t = pkg.capi.PositionTracker(capacity=64, receivers=[None, None], host=True)
    b = ps.Builder(pkg)
    b.pos(ps.T0, 0xABCDEF, 10.0, 10.0, 0).pos(ps.T0 + 100, 0xABCDEF, 10.0, 10.0, 1, rx=1)
    _, m, f, r = b.step()
    assert len(t.update(m[:0], f[:0], r[:0])) == 0                     # n == 0
    assert t.f["update"](t.h, None, None, None, 0, None) == 0          # ... whatever the pointers are
    assert t.f["update"](t.h, None, f.ctypes.data, None, 2, m.ctypes.data) == -errno.EINVAL
    assert t.f["update"](t.h, m.ctypes.data, f.ctypes.data, None, 2, None) == -errno.EINVAL
    bad = np.array([0, 2], dtype=np.uint32)
    with pytest.raises(pkg.MsdError) as e:
        t.update(m, f, bad)
    assert e.value.code == -errno.EINVAL and t.stats()["aircraft"] == 0  # nothing changed
    assert t.f["set_receiver"](t.h, 2, None) == -errno.EINVAL
    out = t.update(m, f, r)                                             # the same address on two receivers: two aircraft
    assert t.stats()["aircraft"] == 2 and [int(x) for x in out["result"]] == [-1, -1]
    t.close()


@pytest.mark.parametrize("sink", ["--net-raw", "--beast", "--no-output"])
@pytest.mark.parametrize("first", [False, True])
def test_replay_refuses_positions_beside_another_sink(pkg, sink, first):
    """--positions prints the --raw lines; with another output chosen, in either order, the tool says so and exits 2
    before it opens a device or a file."""
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "msd_replay")
    args = [sink, "--positions"] if first else ["--positions", sink]
    res = subprocess.run([exe, "--ifile", "/nonexistent"] + args, capture_output=True, text=True, timeout=30)
    assert res.returncode == 2 and "--positions" in res.stderr and not res.stdout
