"""xec_repair's host scan (xec_scan_repair, csrc/xec_scan.cpp) under
AddressSanitizer + UBSan, as a stand-alone program with exact-size buffers,
built exactly as tests/host/scan_fuzz.cpp is (tests/test_host_sanitizers.py):
verdict, item count and item values -- parity items included -- against a plain
per-stripe loop, at row widths 1...257."""
from __future__ import annotations

import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_repair_scan_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "repair_scan_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "host" / "repair_scan_fuzz.cpp"),
                    str(ROOT / "erasure-code-benchmark_amd" / "csrc" / "xec_scan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "repair_scan_fuzz ok" in p.stdout
