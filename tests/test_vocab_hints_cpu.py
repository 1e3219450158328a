"""The vocab-entry hint functions of emqx_amd/csrc/tm_layout.h on the CPU.

tests/hints_cpu/hints_check.cpp is a stand-alone program (own main) over the
shared header alone:

* for random child summaries (flags of the child and of its '+' child, Blooms of
  random child sets up to and past saturation, and arbitrary 64-bit values),
  levels and next words: hint_alive(hint_of_sum(s)) false implies child_alive(s)
  false; a live slot's hint is never the "no child" value 0; every child word's
  bit is set in the hint's folded Bloom;
* vocab_short_eq accepts exactly equal (len, b0, b1) whatever the tag's hint
  bits hold, and a long word's tag can never pass for a short one.

Built with -fsanitize=address,undefined; nothing is loaded into Python.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "hints_cpu" / "hints_check.cpp"


def test_hint_alive_shadows_child_alive(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build the hint check")
    exe = tmp_path / "hints_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "hints ok" in r.stdout
