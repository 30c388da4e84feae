#!/usr/bin/env python3
"""sha256 of the device assembly of every translation unit of the library, as build.py compiles it (FLAGS + EXTRA_FLAGS +
--cuda-device-only -S), lines with the source-text hash symbol __hip_cuid_ removed; the FFT-psd units a second time as
the program_order variant builds them.  Two trees whose digests agree ship the same kernels: run it in both (no GPU).
   tools/isa_digest.py [-k DIR]      one line "<sha256>  <unit>" per unit; -k keeps the filtered assembly in DIR
"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdrainer_amd.csrc import build  # noqa: E402

keep = sys.argv[sys.argv.index("-k") + 1] if "-k" in sys.argv else None
units = [(s, s, []) for s in build.SOURCES]
units += [(s + " -USDR_SAFE_FENCES", s, build.VARIANTS["program_order"]) for s in ("k_fft_psd.hip", "k_fft_psd_win.hip")]


def digest(unit):
    name, src, extra = unit
    cmd = [build.hipcc()] + build.FLAGS + extra + build.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, cwd=build.HERE, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    asm = b"".join(line for line in asm.splitlines(keepends=True) if b"__hip_cuid_" not in line)
    if keep:
        os.makedirs(keep, exist_ok=True)
        with open(os.path.join(keep, name.replace(" ", "_") + ".s"), "wb") as f:
            f.write(asm)
    return hashlib.sha256(asm).hexdigest()


with concurrent.futures.ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
    for unit, d in zip(units, pool.map(digest, units)):
        print(f"{d}  {unit[0]}")
