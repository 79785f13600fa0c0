"""Every device header of tinycarlo_amd/csrc (k_*.h) compiles when it is the only thing a .hip file
includes: each includes what it uses and none relies on what tinycarlo_hip.hip happened to include before it.  No GPU
needed: hipcc checks the device side's syntax for gfx950, once plain and once as the timing build (whose probes are code).
The HIP-free tc_*.h beside them are built alone by their own tests, with the host compiler."""
import glob
import os
import re
import subprocess

import pytest

from common import HIPCC, ROOT

CSRC = os.path.join(ROOT, "tinycarlo_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "k_*.h")))
# the Makefile's language flags (optimisation and output flags play no part in a syntax check)
FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function", "-I", CSRC]


def test_the_source_includes_exactly_the_device_headers():
    """the glob above is the set of device headers: what tinycarlo_hip.hip includes, no more and no less"""
    with open(os.path.join(CSRC, "tinycarlo_hip.hip")) as f:
        included = re.findall(r'^#include "(k_\w+\.h)"$', f.read(), re.M)
    assert HEADERS and sorted(included) == HEADERS, (included, HEADERS)


@pytest.mark.parametrize("define", [None, "-DTC_TIMING"], ids=["plain", "timing"])
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(tmp_path, header, define):
    src = tmp_path / "one.hip"
    src.write_text('#include "%s"\n' % header)
    cmd = [HIPCC, *FLAGS, *([define] if define else []), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
