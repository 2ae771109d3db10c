"""Host-only fuzz of the write scan (xec_scan_write_items, csrc/xec_scan.cpp)
under AddressSanitizer + UBSan -- needs g++ but no GPU and no HIP.  A
stand-alone program with its own main: bitmap, items and bits in exact-size
heap allocations, 20,000 random cases, verdict, counts and every item's two
bits compared with a naive restatement."""
from __future__ import annotations

import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_write_scan_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "write_scan_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "host" / "write_scan_fuzz.cpp"),
                    str(ROOT / "erasure-code-benchmark_amd" / "csrc" / "xec_scan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "write_scan_fuzz ok: 20000 cases" in p.stdout
