"""The tokeniser's word-at-a-time scan (emqx_amd/csrc/tm_scan.h) on the CPU.

tests/scan_cpu/scan_check.cpp is a stand-alone program (own main) that runs the
scan header and the byte loop it replaced, kept in that file as the reference,
over the same inputs and compares level count, every stored level's
(b0, b1, len) or (len, start, 255), `bad`, the '$' flag and the early exit:

* every string over {a, /, +, #, $} up to 7 bytes at all 16 start alignments;
* seeded random topics up to 300 bytes: word lengths 0-20, up to 70 levels;
* seeded random topics up to 300 bytes over all 256 byte values (NUL, the
  high-bit twins of '/', '+', '#', '$' and the neighbours of '/' more often);
* stores of 2, 8 and 32 levels, with and without NEED;
* slash_mask16 alone against a byte loop: every pair of byte values at every
  pair of adjacent positions of a chunk.

Buffers are padded to a 16-byte multiple and its byte source aborts on a load
that is not an aligned granule holding a byte of the topic.  Built with
-fsanitize=address,undefined; nothing is loaded into Python.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "scan_cpu" / "scan_check.cpp"


def test_scan_matches_byte_loop(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build the scan check")
    exe = tmp_path / "scan_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "scan ok" in r.stdout
