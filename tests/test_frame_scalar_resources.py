"""The compiler's record of the five-wave frame kernel's scalar-register spills (no GPU: hipcc cross-compiles gfx950 to assembly).

A spilled scalar register is a v_writelane where it is set aside and a v_readlane where it comes back -- vector instructions, in
a kernel that is bound by vector issue.  Round 16 left tc_frame_kernel<5, true, 1, 32> with 159 of them (99 before it); with
the camera's K matrix fetched at the projection and the raster stage's one-band form it has 37, and tc_frame_banded, the
same kernel with the band loop, 54.  The bound of 60 holds both well under what they were.  Only the metadata fields of the
code object are read, as tests/common.py::dev_kernel_resources reads them (it does not return the scalar spill count)."""
import os
import re
import subprocess
import tempfile

import pytest

from common import HIPCC, ROOT

FRAME = "_Z15tc_frame_kernelILi5ELb1ELi1ELi32EEv9FrameArgs"            # tc_frame_kernel<5, true, TC_FMT_CLASSES, 32>
BANDED = "_Z15tc_frame_bandedILi5ELb1ELi1ELi32EEv9FrameArgs"           # tc_frame_banded<5, true, TC_FMT_CLASSES, 32>
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def dev_metadata():
    """{mangled name: {field: value}} of every kernel of the -DTC_DEV_FAST build (the flags of dev_kernel_resources)"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "tc.s")
        cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-mllvm", "-disable-machine-licm", "-std=c++17",
               "-DTC_DEV_FAST", "-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "tinycarlo_amd", "csrc", "tinycarlo_hip.hip")]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL, timeout=900)
        with open(out) as f:
            s = f.read()
    seen = {}
    for b in s.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        seen[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", b).group(1)) for k in FIELDS}
    return seen


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_five_wave_frame_kernels_keep_their_scalars():
    seen = dev_metadata()
    # the kernel and every instantiation that exists for its sake: the dev set has exactly these two of the K = 5 / 32 frame form
    mine = sorted(n for n in seen if re.match(r"_Z\d+tc_frame(_kernel|_banded)I", n))
    assert mine == sorted([FRAME, BANDED]), mine
    for n in mine:
        m = seen[n]
        assert m["vgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_count"] <= 96, (n, m)
        assert m["sgpr_spill_count"] <= 60, (n, m)
