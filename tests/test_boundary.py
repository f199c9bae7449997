"""The reference-shaped host boundary (include/modes_hip_readsb.h) seen from C written against the
reference's own declarations: tests/c/boundary_check.c must compile with -Werror -- the exported
converter factory is assignable to the reference's iq_convert_fn / init_converter types, the ifile
handler takes the reference's option keys through msd_ifileSetOptionKeys -- and run."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readsb-protobuf_amd", "csrc")


def build_check(tmp_path, libdir=CSRC):
    exe = str(tmp_path / "boundary_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "boundary_check.c"), "-o", exe, "-L" + libdir, "-lmsd_host",
                           "-lmodes_hip", "-Wl,-rpath," + libdir, "-lpthread", "-lm"])
    return exe


RECORDED_LAYOUT = os.path.join(ROOT, "tests", "golden", "reference_boundary.json")


def reference_headers(oracle):
    """The reference tree whose fifo.h / convert.h / demod_2400.h the checks below compile against, or None where the
    checkout has no reference tree beside it."""
    return oracle.REF_DIR if os.path.exists(os.path.join(oracle.REF_DIR, "fifo.h")) else None


def dump_layout(tmp_path, ref=None):
    """tests/c/boundary_layout_dump.c: the mag_buf layout of this library's header, or with ref of the reference's."""
    exe = str(tmp_path / ("layout_ref" if ref else "layout_ours"))
    extra = ["-DDUMP_REFERENCE", "-I" + ref] if ref else []
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")] + extra +
                          [os.path.join(ROOT, "tests", "c", "boundary_layout_dump.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True)
    return json.loads(out.stdout)


def test_boundary_is_pinned_on_the_references_own_header_text(pkg, oracle, tmp_path):
    """convert.h, fifo.h and demod_2400.h are self-contained (fifo.h:57-120, convert.h:27-45, demod_2400.h:37-38).
    `struct msd_mag_buf` has the layout of the reference's `struct mag_buf` field by field, and the same flag and format
    values, as recorded from those headers in tests/golden/reference_boundary.json.  Where the reference tree is there,
    the record is checked against it, one translation unit compares the two structs and the threshold values with
    static asserts, and the other assigns every replacement entry point to a pointer of the reference's declared type
    without a cast under -Werror and runs the FIFO through those pointers."""
    with open(RECORDED_LAYOUT) as f:
        want = json.load(f)
    thresholds = {k: want.pop(k) for k in list(want) if k.startswith("PREAMBLE_THRESHOLD_")}
    assert dump_layout(tmp_path) == want
    # the thresholds the C-ABI documents (msd_config.preamble_threshold, MSD_MAX_PREAMBLE_THRESHOLD) are the reference's
    assert thresholds == {"PREAMBLE_THRESHOLD_DEFAULT": 58, "PREAMBLE_THRESHOLD_MIN": 40, "PREAMBLE_THRESHOLD_MAX": 400,
                          "PREAMBLE_THRESHOLD_PIZERO": 75}
    REF = reference_headers(oracle)
    if REF is None:
        return
    assert dump_layout(tmp_path, REF) == {**want, **thresholds}  # the record still is the reference's layout
    for name, libs in (("boundary_ref_layout", []),
                       ("boundary_ref_bind", ["-L" + CSRC, "-lmsd_host", "-lmodes_hip", "-Wl,-rpath," + CSRC, "-lpthread", "-lm"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + REF,
                               os.path.join(ROOT, "tests", "c", name + ".c"), "-o", exe] + libs)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and " ok" in out.stdout, (name, out.returncode, out.stdout + out.stderr)


def test_reference_types_are_bound_by_explicit_opt_in_only(oracle, tmp_path):
    """Round 6: which types the header declares its entry points with follows the includer's
    MSD_BIND_REFERENCE_* macros, not the reference's include guards.  Without the reference's headers the library's own
    types compile and the opt-in does not (a missing reference header is a compile error).  Where the reference tree is
    there: behind the reference's headers WITHOUT the macro the library's own struct is declared (msd_fifo_acquire does
    not return a `struct mag_buf *`: -Werror refuses the assignment); with the macro the same line compiles; and the
    converter and the FIFO opt in separately."""
    REF = reference_headers(oracle)

    def compiles(defs, body, ref_headers=True):
        src = tmp_path / "optin.c"
        src.write_text('#include <stdint.h>\n' + ('#include "convert.h"\n#include "fifo.h"\n' if ref_headers else "") + defs +
                       '\n#include "modes_hip_readsb.h"\n' + body + "\nint main(void) { return 0; }\n")
        return subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] +
                              (["-I" + REF] if ref_headers else []) + [str(src)], capture_output=True, text=True).returncode == 0
    own = "struct msd_mag_buf *(*const p)(uint32_t) = msd_fifo_acquire; void *use_p(void) { return (void *)p; }"
    assert compiles("", own, ref_headers=False)
    assert not compiles("#define MSD_BIND_REFERENCE_FIFO 1", "", ref_headers=False)
    assert not compiles("#define MSD_BIND_REFERENCE_CONVERTER 1", "", ref_headers=False)
    if REF is None:
        return
    fifo_line = "struct mag_buf *(*const p)(uint32_t) = msd_fifo_acquire; void *use_p(void) { return (void *)p; }"
    conv_line = "__typeof__(&init_converter) const q = msd_init_converter; void *use_q(void) { return (void *)q; }"
    assert not compiles("", fifo_line) and not compiles("", conv_line)           # the guards FIFO_H / CONVERT_H are in scope: no effect
    assert compiles("#define MSD_BIND_REFERENCE_TYPES", fifo_line + conv_line)
    assert compiles("#define MSD_BIND_REFERENCE_FIFO 1", fifo_line) and not compiles("#define MSD_BIND_REFERENCE_FIFO 1", conv_line)
    assert compiles("#define MSD_BIND_REFERENCE_CONVERTER 1", conv_line) and not compiles("#define MSD_BIND_REFERENCE_CONVERTER 1", fifo_line)
    assert compiles("", own)                                                       # the library's own types beside the reference's


def test_boundary_compiles_against_reference_style_declarations_and_runs(pkg, tmp_path):
    exe = build_check(tmp_path, os.path.dirname(pkg.capi.LIB_PATH))   # (a sanitizer build when tests/test_sanitizers.py runs this)
    capture = tmp_path / "tiny.uc8"
    np.full(2 * 4096, 127, dtype=np.uint8).tofile(capture)
    out = subprocess.run([exe, str(capture)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "boundary ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_boundary_check_on_the_gpu(pkg, tmp_path, torch_cuda):
    """With a device: the converter obtained through the reference-typed factory converts, the handler
    runs a capture to its end and calls the exit / monitor / EOF hooks."""
    exe = build_check(tmp_path)
    capture = tmp_path / "small.uc8"
    rng = np.random.default_rng(3)
    rng.integers(100, 156, size=2 * (131072 + 5000), dtype=np.uint8).tofile(capture)
    out = subprocess.run([exe, str(capture)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "boundary ok" in out.stdout, out.stdout + out.stderr
