"""The position tracker's stream writers past one round of their scan: the GPU object against the host twin, byte for
byte, at the three shapes of tests/writer_scale.py.  Every writer lays its stream out by one workgroup's scan over the
other workgroups' sums (msd_block_scan_impl.h: block_sums_scan), 256 sums a round; up to 65 536 records or items the loop
runs once and what it carries from round to round is never used, and no other test of these writers goes further.
Here the reduced Beast and the SBS writer see 263 172 records (five rounds), aircraft.pb and the VRS list 65 796 to
133 377 items (two and three rounds, aircraft.pb through scan_kernel<4>'s four strided arrays), and the range's
Statistics.polar_range 4 718 592 entries (72 rounds).  The conditions on the twin's own output -- that the shapes are what
they are meant to be, and that no margin is near -- are those of tests/test_writer_scale_model.py."""
import pytest

import writer_scale as ws

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_gpu_equals_twin(pkg, torch_cuda, shape):
    """a: records past one round (65 793 aircraft on 3 receivers, 263 172 records, every writer); b: items past two
    rounds and 1 024 files (131 329 aircraft); c: 65 536 receivers and 300 aircraft, with the range."""
    stream = getattr(ws, "stream_" + shape)(pkg)
    run = getattr(ws, "run_" + shape)
    want = run(pkg, stream, True)
    getattr(ws, "shape_" + shape)(pkg, stream, want)
    got = run(pkg, stream, False)
    for name in ws.COMPARED[shape]:
        diff = ws.first_difference(name, got[name], want[name])
        assert diff is None, diff
    assert got["live"] == want["live"]
