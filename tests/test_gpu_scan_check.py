"""The scan every stream writer lays its output out by (msd_block_scan_impl.h: block_scan and block_sums_scan, through
msd_wire_store_impl.h's scan_kernel<1> and <4>), alone and against a 64-bit prefix sum on the host
(scripts/micro/scan_check.hip): 1 to 65 537 workgroup sums -- from 257 on every offset rests on the carry between the
rounds of 256 -- random, all zero and with a grand total of exactly 2^32 - 1, guard words either side of the arrays, and
block_scan called twice on the same LDS words.  The program first shows, on host arrays it made wrong, that its
comparison names the first differing word."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_scan_kernels_equal_a_host_prefix_sum(torch_cuda, tmp_path):
    exe = str(tmp_path / "scan_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3",
                           "-I" + os.path.join(ROOT, "readsb-protobuf_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "scripts", "micro", "scan_check.hip"), "-o", exe], timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    m = re.search(r"^(\d+) cases, 0 differ$", out.stdout, re.M)
    assert out.returncode == 0 and m, out.stdout + out.stderr
    # 10 sizes x 3 kinds of values x scan_kernel<1>, <4>, and block_scan's workgroups twice each
    assert int(m.group(1)) == 10 * 3 * 2 + 24 * 2, out.stdout
    assert "names the first differing word" in out.stdout, out.stdout
