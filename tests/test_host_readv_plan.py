"""Host-only fuzz of the vectored read's plan (xec_plan_readv,
csrc/xec_scan.cpp) under AddressSanitizer + UBSan -- needs g++ but no GPU and
no HIP.  A stand-alone program with its own main: bitmap, entries and table in
exact-size heap allocations, tile sizes 1 to 8 KiB, list lengths at 0, 1 and
around the kernel-argument capacities, every prefix, column, loss bit and
tile-to-entry lookup compared with a direct loop."""
from __future__ import annotations

import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_readv_plan_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "readv_plan_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "host" / "readv_plan_fuzz.cpp"),
                    str(ROOT / "erasure-code-benchmark_amd" / "csrc" / "xec_scan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "readv_plan_fuzz ok: 1400 cases" in p.stdout
