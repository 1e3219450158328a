"""The retained store's host side (emqx_amd/csrc/tm_retain_host.cpp) on the CPU
device fake, under AddressSanitizer and UndefinedBehaviorSanitizer.

tests/retain_cpu/retain_check.cpp is a stand-alone program (own main) linked
from tm_retain_host.cpp itself, tests/host_cpu/fake_hip.cpp (the hip* functions
over malloc'd memory: every read or write past a "device" array is seen) and
tests/retain_cpu/fake_retain_launch.cpp (the four tmx::launch_ret_* symbols).

The fake's match launchers ignore what the host promises about ranges: they
test every row of the image with a plain restatement of emqx_topic:match/2 over
ids and abort unless that set is the one found inside the segments the filter
was handed, and the one the kernel's shortened test (levels past the prefix
only) finds there.  A wrong prefix range, a stale live bit or a row missing
from the tail fails here, without a GPU.  Its apply launcher is k_ret_apply's
definition, with one write per row and launch asserted.  The driver compares
every list with a model keyed by topic string, and covers: growth across
initial_rows, compaction at tail_max = 4, delete then put again in the base and
in the tail, dictionary ids freed and used again (`words` back at its baseline
after 3 * tail_max distinct words were put, deleted and compacted), topics of 9
and 12 levels, both expiry rules, tm_retained_expire, six seeded churn scripts,
segments of several tiles in the base and in the tail, and no live allocation
after the last destroy.  The program is built a second time with
RT_LAUNCH_TILES = 3, so that every batch is scanned by several launches with a
tile offset each (the product's launches take 2^24 - 1 tiles: HIP launches
fewer than 2^32 threads); the fake refuses a launch of 2^32 threads or more, of
more than RT_LAUNCH_TILES tiles, and a gap or an overlap between a batch's
launches.  Nothing is loaded into Python; no LD_PRELOAD.
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
    pytest.fail("no HIP headers (hip/hip_runtime_api.h) to compile tm_retain_host.cpp against")


def _build(tmp_path_factory, name, defines):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build the retain check")
    out = tmp_path_factory.mktemp(name)
    inc = ["-I", str(_hip_include())]
    units = [(ROOT / "emqx_amd" / "csrc" / "tm_retain_host.cpp", ["-Wall"]), (ROOT / "tests" / "host_cpu" / "fake_hip.cpp", OWN),
             (ROOT / "tests" / "retain_cpu" / "fake_retain_launch.cpp", OWN), (ROOT / "tests" / "retain_cpu" / "retain_check.cpp", OWN)]
    procs = [(src, subprocess.Popen([cxx, *BASE, *SAN, *defines, *extra, *inc, "-c", str(src), "-o", str(out / f"{src.stem}.o")],
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for src, extra in units]
    for src, p in procs:
        log, _ = p.communicate()
        assert p.returncode == 0, f"{src.name}:\n{log[-6000:]}"
    exe = out / "retain_check"
    b = subprocess.run([cxx, SAN[0], "-o", str(exe), *[str(out / f"{s.stem}.o") for s, _ in units], "-lpthread"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "retain_check", [])


@pytest.fixture(scope="module")
def program_small_launches(tmp_path_factory):
    """the host side and the fake built with RT_LAUNCH_TILES = 3: every batch of more than three tiles goes out in
    several launches, filters straddle them, and the fake refuses a launch of more tiles, a gap or an overlap"""
    return _build(tmp_path_factory, "retain_check_lt3", ["-DRT_LAUNCH_TILES=3"])


def test_retain_check_with_launches_of_three_tiles(program_small_launches):
    r = subprocess.run([str(program_small_launches)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "retain check ok" in r.stdout


def test_the_launch_bound_is_below_2_32_threads():
    """HIP launches fewer than 2^32 threads (gridDim.x * blockDim.x); the product's bound, from the header"""
    import re
    dev = (ROOT / "emqx_amd" / "csrc" / "tm_retain.h").read_text()
    m = re.search(r"#define RT_LAUNCH_TILES \(\(1u << (\d+)\) - 1\)", dev)
    tile = int(re.search(r"RT_TILE = (\d+);", dev).group(1))
    assert m and ((1 << int(m.group(1))) - 1) * tile < 1 << 32
    assert "static_assert((uint64_t)RT_MAX_LAUNCH_TILES * RT_TILE < (1ull << 32)" in dev
    host = (ROOT / "emqx_amd" / "csrc" / "tm_retain_host.cpp").read_text()
    assert host.count("t0 += RT_MAX_LAUNCH_TILES") == 2, "the count and the emit pass both go out in runs of tiles"


def test_retain_check_under_the_sanitizers(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "retain check ok" in r.stdout
