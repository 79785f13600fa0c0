"""The compiler's record of the kernels the cull verdict in the pose row touches (no GPU: hipcc cross-compiles gfx950 to
assembly, with the flags of tests/test_frame_scalar_resources.py, whose reader of the metadata this uses).

The frame kernels lost the predicate and tc_frame_kernel<5, true, 1, 32> the camera group loop: it had 37 spilled scalar
registers before and may not have more (it has none).  The simulate kernels gained the predicate at their pose-row stores;
they sit at 123 to 128 VGPRs -- four wavefronts per SIMD -- and must not cross that, and no frame or simulate kernel may spill
a vector register or use scratch."""
import os
import re

import pytest

from common import HIPCC
from test_frame_scalar_resources import FRAME, dev_metadata

SPILLS_BEFORE = 37
FAMILIES = r"_Z\d+tc_(frame_kernel|frame_banded|frame_recover_kernel|envg_kernel|drive_envg_kernel|env_kernel|drive_env_kernel)I"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_frame_and_simulate_kernels_keep_their_registers():
    seen = dev_metadata()
    assert seen[FRAME]["sgpr_spill_count"] <= SPILLS_BEFORE, seen[FRAME]
    mine = sorted(n for n in seen if re.match(FAMILIES, n))
    # the frame kernel, its banded twin and the recover kernel; the grouped simulate kernels with and without the controller
    # (four feature masks each); the per-env ones with and without the camera stage
    assert len([n for n in mine if "tc_frame" in n]) == 3 and len([n for n in mine if "envg_kernel" in n]) == 8, mine
    assert len([n for n in mine if re.match(r"_Z\d+tc_(drive_)?env_kernelI", n)]) == 16, mine
    for n in mine:
        m = seen[n]
        assert m["vgpr_spill_count"] == 0, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_count"] <= 128, (n, m)
