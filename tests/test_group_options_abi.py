"""Per-receiver options of receiver groups at the C-ABI, without a device: libmodes_hip.so exports both entries,
msd_group_receiver_options has the layout modes_hip.h documents, and capi mirrors it."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("preamble_threshold", 0, 4), ("nfix_crc", 4, 4), ("reserved", 8, 8)]


def test_library_exports_the_option_entries(pkg):
    lib = pkg.capi.lib()
    for name in ("msd_group_set_receiver_options", "msd_group_get_receiver_options"):
        assert hasattr(lib, name), name
        assert name in pkg.capi.EXPORTS


def test_header_layout(tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("{f} %zu %zu\\n", offsetof(msd_group_receiver_options, {f}), '
                   f'sizeof(((msd_group_receiver_options *)0)->{f}));\n' for f, _, _ in FIELDS)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"modes_hip.h\"\nint main(void)\n{\n"
                   '    printf("size %zu\\n", sizeof(msd_group_receiver_options));\n' + body + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    got = dict((w[0], tuple(int(x) for x in w[1:])) for w in
               (line.split() for line in subprocess.check_output([exe], text=True).splitlines()))
    assert got["size"] == (16,)
    for f, off, size in FIELDS:
        assert got[f] == (off, size), f


def test_capi_mirrors_the_struct(pkg):
    O = pkg.capi.GroupReceiverOptions
    assert C.sizeof(O) == 16
    assert [n for n, _ in O._fields_] == [f for f, _, _ in FIELDS]
    for f, off, size in FIELDS:
        assert getattr(O, f).offset == off and getattr(O, f).size == size, f
    o = O(75, 2)
    assert (o.preamble_threshold, o.nfix_crc, list(o.reserved)) == (75, 2, [0, 0])
