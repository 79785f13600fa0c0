#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the device code of two builds of the HIP library (no GPU needed).

    python tools/device_code_identity.py PARENT_BUILD_DIR NEW_BUILD_DIR

Each directory holds part0.o .. part5.o of `make` (tinycarlo_amd/csrc/build).  From every object the gfx950 code object is
unbundled, and for every kernel symbol the bytes of its code and its metadata note entry are hashed.  Prints one line per
kernel that differs or exists on one side only, and the count of identical ones per part."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def kernels(obj, td, tag):
    co, fat = os.path.join(td, tag + ".co"), os.path.join(td, tag + ".fatbin")
    subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj])  # the bundle inside the host object
    subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    sec = subprocess.run([LLVM + "llvm-readelf", "-S", "--wide", co], capture_output=True, text=True, check=True).stdout
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    blob = open(co, "rb").read()
    out = {}
    sym = subprocess.run([LLVM + "llvm-readelf", "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
    for line in sym.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            a, n = int(f[1], 16), int(f[2], 0)
            out[f[7]] = (n, hashlib.sha256(blob[off + a - addr: off + a - addr + n]).hexdigest())
    return out


def main():
    pa, nw = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as td:
        for p in range(6):
            a = kernels(os.path.join(pa, "part%d.o" % p), td, "a%d" % p)
            b = kernels(os.path.join(nw, "part%d.o" % p), td, "b%d" % p)
            same = 0
            for k in sorted(set(a) | set(b)):
                if a.get(k) == b.get(k):
                    same += 1
                    continue
                name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
                name = re.sub(r"\(.*\)$", "", name).replace("void ", "")
                print("part%d  DIFFERS  %-60s parent %s  new %s" % (p, name, a.get(k, ("-",))[0], b.get(k, ("-",))[0]))
            print("part%d  %d kernels byte-identical (code bytes, by symbol)" % (p, same))


if __name__ == "__main__":
    main()
