"""tm_retained_match_page, tm_retained_pin and tm_retained_unpin
(emqx_amd/csrc/tm_retain_page_host.cpp) on the CPU device fake, under
AddressSanitizer and UndefinedBehaviorSanitizer.

tests/retain_cpu/retain_page_check.cpp is a stand-alone program (own main)
linked from tm_retain_host.cpp and tm_retain_page_host.cpp themselves,
tests/host_cpu/fake_hip.cpp (the hip* functions over malloc'd memory: every read
or write past a "device" array is seen), tests/retain_cpu/fake_retain_launch.cpp
unchanged (launch_ret_offsets is used by the page path) and
tests/retain_cpu/fake_retain_page_launch.cpp, which restates the three page
kernels in plain C++.

The fake page launcher does not trust the host: for every filter it tests every
row of the image with a plain restatement of emqx_topic:match/2 over ids and
aborts unless the matching rows from the cursor to the window's end, cut at
`limit`, are exactly the values the segments it was handed produce, in scan
order; a gap or an overlap between a batch's launches is refused.  The driver
compares every drain with a model keyed by topic string and covers: drains at
limits 1, 255, 256, 257, 1000 and mid-tile over stores in the tail, in the base
and across both, put order with an empty base, the tile edges, hits in single
waves, a cursor handed to another filter, 64 filters at mixed positions,
capacity, expiry, dead rows and '$' topics, scan windows, pins (also under two
threads), stale cursors, six seeded churn scripts, and no live allocation after
the last destroy.  The program is built a second time with RT_LAUNCH_TILES = 3.
Nothing is loaded into Python; no LD_PRELOAD.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BASE = ["-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OWN = ["-Wall", "-Wextra", "-Werror"]   # the test's own files only


def _hip_include():
    for p in (Path("/opt/rocm/include"), Path(shutil.which("hipcc") or "/nonexistent").resolve().parent.parent / "include"):
        if (p / "hip" / "hip_runtime_api.h").exists():
            return p
    pytest.fail("no HIP headers (hip/hip_runtime_api.h) to compile tm_retain_page_host.cpp against")


def _build(tmp_path_factory, name, defines):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build the retain page check")
    out = tmp_path_factory.mktemp(name)
    inc = ["-I", str(_hip_include())]
    csrc, cpu = ROOT / "emqx_amd" / "csrc", ROOT / "tests" / "retain_cpu"
    units = [(csrc / "tm_retain_host.cpp", ["-Wall"]), (csrc / "tm_retain_page_host.cpp", ["-Wall"]),
             (ROOT / "tests" / "host_cpu" / "fake_hip.cpp", OWN), (cpu / "fake_retain_launch.cpp", OWN),
             (cpu / "fake_retain_page_launch.cpp", OWN), (cpu / "retain_page_check.cpp", OWN)]
    procs = [(src, subprocess.Popen([cxx, *BASE, *SAN, *defines, *extra, *inc, "-c", str(src), "-o", str(out / f"{src.stem}.o")],
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for src, extra in units]
    for src, p in procs:
        log, _ = p.communicate()
        assert p.returncode == 0, f"{src.name}:\n{log[-6000:]}"
    exe = out / "retain_page_check"
    b = subprocess.run([cxx, SAN[0], "-o", str(exe), *[str(out / f"{s.stem}.o") for s, _ in units], "-lpthread"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "retain_page_check", [])


@pytest.fixture(scope="module")
def program_small_launches(tmp_path_factory):
    """the host side and the fakes built with RT_LAUNCH_TILES = 3: every page batch of more than three tiles goes
    out in several launches per pass, and the fake refuses a launch of more tiles, a gap or an overlap"""
    return _build(tmp_path_factory, "retain_page_check_lt3", ["-DRT_LAUNCH_TILES=3"])


def test_retain_page_check_under_the_sanitizers(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "retain page check ok" in r.stdout


def test_retain_page_check_with_launches_of_three_tiles(program_small_launches):
    r = subprocess.run([str(program_small_launches)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "retain page check ok" in r.stdout


def test_the_store_file_calls_no_page_launcher_and_the_page_file_goes_out_in_runs():
    host = (ROOT / "emqx_amd" / "csrc" / "tm_retain_host.cpp").read_text()
    page = (ROOT / "emqx_amd" / "csrc" / "tm_retain_page_host.cpp").read_text()
    assert "launch_retp_" not in host and "tm_retain_page.h" not in host
    assert page.count("t0 += RT_MAX_LAUNCH_TILES") == 2, "the count and the emit pass both go out in runs of tiles"
    kern = (ROOT / "emqx_amd" / "csrc" / "tm_retain_page.hip").read_text()
    assert "atomic" not in kern.split("#include", 1)[1] and "asm" not in kern.split("#include", 1)[1]
