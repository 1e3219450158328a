"""The host side of tm_set_subscribers (emqx_amd/csrc/tm_subs.h) on the CPU.

tests/subs_cpu/subs_check.cpp is a stand-alone program (own main) that drives
the header with 120,000 seeded set / replace / clear operations (lists of 0-3
ids mostly, 1000-4000 now and then, phases of clears) against a std::map model:

* every live span lies inside the pool, no two live spans overlap, every list
  equals the model's;
* a copy that takes only the dirty ranges after each operation equals the host
  arrays word for word;
* compaction happens, preserves every list and leaves a pool of at most
  2 x the live words + one block; after every call the garbage is at most the
  live words.

Built with -fsanitize=address,undefined; nothing is loaded into Python.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "subs_cpu" / "subs_check.cpp"


def test_subscriber_pool_against_a_map(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build the subscriber pool check")
    exe = tmp_path / "subs_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "subs ok" in r.stdout


def test_the_header_is_not_a_kernel_source():
    from emqx_amd import build
    assert "tm_subs.h" not in build.KERNEL_SOURCES and build.DISPATCH_SOURCE not in build.KERNEL_SOURCES
