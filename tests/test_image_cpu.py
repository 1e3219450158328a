"""The host index compiler (emqx_amd/csrc/tm_host.cpp) on a CPU device fake, under
AddressSanitizer and UndefinedBehaviorSanitizer, with an audit of the image.

tests/host_cpu/image_check.cpp is a stand-alone program (own main) linked from
tm_host.cpp itself, fake_hip.cpp (the 28 hip* functions it calls, over malloc'd
memory: every read or write past a "device" table is seen) and fake_launch.cpp
(the 28 tmx:: symbols).  It runs the scenario files of tests/image_script.py
through the public ABI of include/tmatch.h with copies 1 and 2 and compares every
check step exactly with the oracle's answers the file carries.

What the fake implements, and what it answers.  launch_match,
launch_match_pairs, launch_first and launch_small_segs run image_walk.h's
reference walker, which decides from the primary structure alone and asserts, at
every child whose subtree gave a hit, that the summary, Bloom bit, bitmap bit and
hint the parent holds say "alive" (audit by use).  launch_patch is k_patch's
definition with every run bounded by the table's allocation; launch_matches_filter
is the ordered filter walk; launch_sort_segments and launch_copy_values exist
because tm_match_batch's sorted orders cannot avoid them.  Every other launcher
answers hipErrorNotSupported, and the driver fails if one was reached.
small_path_ok answers false for the staged and in-place tm_match_batch /
tm_first_batch calls (they take launch_match / launch_first) and true for
tm_match_batch32_ex / tm_match_batch32_pairs (through the combiner to
launch_small_segs); the driver asserts the path counters moved accordingly.
hipEventQuery answers hipErrorNotReady for as many calls as the driver asks:
tm_commit's wait loop, its forced path and lane_busy are reached, and asserted
through TM_DEBUG_COMMIT_WAITS / TM_DEBUG_COMMIT_FORCED.

After every check step the full audit recomputes every derived word of the view
the launch was given -- psum, CSlot.sum, nlit, wide bitmaps, the hint fields of
every annex slot that is held (a released slot's bits are left as they are and
nothing reads them, tm_host.cpp annex_set: not looked at), annex flags and depths, xfp, stored hashes and tags, reachability in vocab, exact
and every child table, value runs inside vals -- and asserts equality; depth,
xlen_mask, xlen_max and hdesc must suffice.  The 192-bit Bloom is asserted as a
superset: child_remove clears no bit (a Bloom cannot forget one word) and only a
table move builds it anew; stale bits are reported.

A scenario that claims an audit kind (wide bitmaps, hints in both slots,
saturated QQ Blooms, wrapped erase runs, both compactions, both table shrinks,
node and wid reuse, more patches per copy than PATCH_RING, a vocab rehash while
both annex slots are held, ...) fails if its count is zero.  The same program is built
a second time under ThreadSanitizer for test_image_threads.  Nothing is loaded
into Python; no LD_PRELOAD.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

import image_script

ROOT = Path(__file__).resolve().parent.parent

SRC = ROOT / "tests" / "host_cpu"
BASE = ["-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__"]
SAN = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}
OWN = ["-Wall", "-Wextra", "-Werror"]   # the test's own files only


def _hip_include():
    for p in (Path("/opt/rocm/include"), Path(shutil.which("hipcc") or "/nonexistent").resolve().parent.parent / "include"):
        if (p / "hip" / "hip_runtime.h").exists():
            return p
    pytest.fail("no HIP headers (hip/hip_runtime.h) to compile tm_host.cpp against")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """image_check built twice, all eight compilations at once: under ASan + UBSan, and under TSan"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build the image check")
    out = tmp_path_factory.mktemp("image_check")
    inc = ["-I", str(_hip_include())]
    units = [(ROOT / "emqx_amd" / "csrc" / "tm_host.cpp", []), (SRC / "fake_hip.cpp", OWN), (SRC / "fake_launch.cpp", OWN),
             (SRC / "image_check.cpp", OWN)]
    procs = [(kind, src, subprocess.Popen([cxx, *BASE, *san, *extra, *inc, "-c", str(src), "-o", str(out / f"{src.stem}.{kind}.o")],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for kind, san in SAN.items() for src, extra in units]
    for kind, src, p in procs:
        log, _ = p.communicate()
        assert p.returncode == 0, f"{src.name} ({kind}):\n{log[-6000:]}"
    exes = {}
    for kind, san in SAN.items():
        exes[kind] = out / f"image_check_{kind}"
        b = subprocess.run([cxx, san[0], "-o", str(exes[kind]), *[str(out / f"{s.stem}.{kind}.o") for s, _ in units], "-lpthread"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stdout + b.stderr
    return exes


_FILES = {}


def _scenario_file(name, tmp_path_factory):
    if name not in _FILES:   # written once, run with both copy counts
        path = tmp_path_factory.mktemp("scenario") / (name + ".tmis")
        image_script.write(image_script.SCENARIOS[name](), path)
        _FILES[name] = path
    return _FILES[name]


@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("name", list(image_script.SCENARIOS))
def test_image_scenario(programs, tmp_path_factory, name, copies):
    path = _scenario_file(name, tmp_path_factory)
    r = subprocess.run([str(programs["asan"]), str(path), str(copies)], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "image check ok" in r.stdout


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_image_threads(programs, kind):
    """Four threads over the fake with two copies and busy events: tm_commit; tm_apply_deltas + tm_sync;
    tm_match_batch; tm_match_batch32_pairs in place through the combiner with a gather window -- 2,000
    operations.  Each writer's delta moves one filter's value from epoch e - 1 to e, so after any whole
    number of deltas a probe topic has exactly one value, never an older one than the reader saw before."""
    r = subprocess.run([str(programs[kind]), "--threads", "2000"], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-8000:]
    assert "image check ok" in r.stdout
