"""tm_dispatch_batch32 without a device: the export, the ABI minor, the debug
keys, the argument check that needs no GPU, and the NIF core's dispatch half
(c_src/tmatch_nif_dispatch.c) against the stand-in libtmatch
(tests/native/fake_tmatch.c + fake_tmatch_route.c + fake_tmatch_dispatch.c):
the slices and deliveries, one rerun per kind of TM_ECAP (cap alone, dcap
alone, both) with sticky sizes, err 4 -> TM_EDEVICE.

The same cases, with tmn_give and the pool's destruction, run once more in a
stand-alone C program (tests/native/nif_dispatch_check.c) built with
-fsanitize=address,undefined and started as a subprocess; nothing sanitised is
loaded into Python.
"""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest

from emqx_amd import _native

ROOT = Path(__file__).resolve().parent.parent
TM_OK, TM_EINVAL, TM_EDEVICE, TM_ECAP = 0, -1, -3, -4
SOURCES = [ROOT / "c_src" / "tmatch_nif_core.c", ROOT / "c_src" / "tmatch_nif_route.c",
           ROOT / "c_src" / "tmatch_nif_dispatch.c", ROOT / "tests" / "native" / "fake_tmatch.c",
           ROOT / "tests" / "native" / "fake_tmatch_route.c", ROOT / "tests" / "native" / "fake_tmatch_dispatch.c"]


def test_export_abi_minor_and_debug_keys():
    lib = _native.load_library()
    assert "tm_dispatch_batch32" in _native.EXPORTS and hasattr(lib, "tm_dispatch_batch32")
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 17
    assert (_native.TM_DEBUG_DISPATCH_ONE, _native.TM_DEBUG_DISPATCH_GRID, _native.TM_DEBUG_DP1_MAX) == (32, 33, 34)
    header = (ROOT / "include" / "tmatch.h").read_text()
    for name, key in (("TM_DEBUG_DISPATCH_ONE", 32), ("TM_DEBUG_DISPATCH_GRID", 33), ("TM_DEBUG_DP1_MAX", 34)):
        assert f"{name} = {key}" in header
    assert "int tm_dispatch_batch32(" in header


def test_null_handle_is_einval():
    lib = _native.load_library()
    offs = (C.c_uint32 * 2)(0, 1)
    doff = (C.c_uint32 * 3)()
    head = (C.c_uint64 * 2)()
    err = (C.c_uint8 * 1)()
    assert lib.tm_dispatch_batch32(None, 1, b"a" * 16, offs, 1, 0, 0, doff, None, None, 0, head, None, None, None, 0,
                                   err) == TM_EINVAL


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("nifdispatch") / "libnifdispatch.so"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out)] + [str(s) for s in SOURCES],
                   check=True)
    lib = C.CDLL(str(out))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    p32, p64 = C.POINTER(u32), C.POINTER(u64)
    lib.fake_pool_new.restype = vp
    lib.fake_pool_free.argtypes = [vp]
    lib.fake_count.restype = C.c_long
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_match.argtypes = [vp, vp, u32, u32]
    lib.tmn_dispatch.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, p64, p64]
    lib.tmn_deliveries.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), C.POINTER(p32), p64]
    for f in (lib.fake_set_vals, lib.fake_set_route_topics):
        f.argtypes, f.restype = [vp], p32
    for f in (lib.fake_set_reruns, lib.fake_set_delivery_cap, lib.fake_set_route_cap):
        f.argtypes, f.restype = [vp], u64
    lib.fake_dispatch_count.restype = C.c_long
    for f in (lib.fake_dispatch_cap, lib.fake_dispatch_dcap):
        f.argtypes, f.restype = [C.c_long], u64
    lib.fake_dispatch_mult.argtypes = [u32]
    yield lib
    lib.fake_dispatch_mult(1)


H = C.c_void_p(1)


def pack(lib, s, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, H, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


def slices(lib, s, n_dests):
    vals, tops = lib.fake_set_vals(s), lib.fake_set_route_topics(s)
    out = []
    for d in range(n_dests + 1):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
        out.append([(tops[k], vals[k]) for k in range(b.value, e.value)])
    return out


def deliveries(lib, s):
    """-> (rc, [(topic, value, subscriber)]) through tmn_deliveries"""
    t, v, d = (C.POINTER(C.c_uint32)() for _ in range(3))
    cnt = C.c_uint64(99)
    rc = lib.tmn_deliveries(s, C.byref(t), C.byref(v), C.byref(d), C.byref(cnt))
    return rc, [(t[k], v[k], d[k]) for k in range(cnt.value)]


def expected(topics, n_dests, local, mult=1):
    """the fakes' rule: value 1000 i + k per byte, bucket v % (n_dests + 1); ((v % 1000) % 7) * mult subscribers"""
    out = [[] for _ in range(n_dests + 1)]
    for i, t in enumerate(topics):
        if t[:1] == b"+":
            continue
        for k in range(len(t)):
            out[(1000 * i + k) % (n_dests + 1)].append((i, 1000 * i + k))
    dl = [(i, v, v * 16 + r) for i, v in out[local] for r in range((v % 1000) % 7 * mult)]
    return out, dl


def test_slices_and_deliveries(core):
    core.fake_dispatch_mult(1)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"abcde", b"+x", b"", b"xyz", b"0123456789"]
    assert pack(core, s, topics) == TM_OK
    for local, flags in ((1, 0), (0, _native.TM_ROUTE_AGGRE), (2, 0)):
        c0 = core.fake_dispatch_count()
        assert core.tmn_dispatch(s, H, len(topics), 3, local, flags) == TM_OK
        assert core.fake_dispatch_count() - c0 == 1 and core.fake_set_reruns(s) == 0
        exp, exp_dl = expected(topics, 3, local)
        assert slices(core, s, 3) == exp and deliveries(core, s) == (0, exp_dl) and len(exp_dl) > 5
    assert core.tmn_dispatch(s, H, len(topics), 3, 3, 0) == TM_EINVAL      # local_dest >= n_dests
    assert deliveries(core, s) == (TM_EINVAL, [])
    assert core.tmn_dispatch(s, H, len(topics), 0, 0, 0) == TM_EINVAL
    # the same set still serves matches/3 (tmn_match) for the packed batch
    assert core.tmn_match(s, H, len(topics), 0) == TM_OK
    core.tmn_give(pool, s)
    a0, f0 = core.fake_count(0), core.fake_count(1)
    core.fake_pool_free(pool)
    assert core.fake_count(1) - f0 >= 11   # blob, offs, hit, vals, err, rdoff, rtopic, dhead, dtopic, dvalue, dsub
    assert core.fake_count(0) == a0


@pytest.mark.parametrize("kind", ["cap", "dcap", "both"])
def test_ecap_reruns_once_and_the_sizes_stick(core, kind):
    """More entries and / or deliveries than the first guess (TMN_IDS_PER_TOPIC per topic +
    1024, and the half tmn_get allocates on top): ONE rerun with room for
    out_dest_offsets[n_dests + 1] entries and out_head[1] deliveries; the second call needs none."""
    topics = [b"abcdefg", b"hijklmn"] if kind == "dcap" else [b"x" * 3000, b"y" * 200]
    mult = {"cap": 1, "dcap": 2000, "both": 40}[kind]
    n_dests, local = (1, 0) if kind == "dcap" else (4, 2)
    core.fake_dispatch_mult(mult)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    assert pack(core, s, topics) == TM_OK
    exp, exp_dl = expected(topics, n_dests, local, mult)
    total, T = sum(map(len, exp)), len(exp_dl)
    c0 = core.fake_dispatch_count()
    assert core.tmn_dispatch(s, H, 2, n_dests, local, 0) == TM_OK
    assert core.fake_dispatch_count() - c0 == 2 and core.fake_set_reruns(s) == 1
    cap0, cap1 = core.fake_dispatch_cap(c0), core.fake_dispatch_cap(c0 + 1)
    dcap0, dcap1 = core.fake_dispatch_dcap(c0), core.fake_dispatch_dcap(c0 + 1)
    assert (cap0 < total) == (kind != "dcap") and (dcap0 < T) == (kind != "cap")
    assert cap1 >= total and dcap1 >= T
    assert (cap1 == cap0) == (kind == "dcap") and (dcap1 == dcap0) == (kind == "cap")   # only what did not fit grew
    assert core.fake_set_route_cap(s) >= 4 * total and core.fake_set_delivery_cap(s) >= 4 * T
    assert slices(core, s, n_dests) == exp and deliveries(core, s) == (0, exp_dl)
    c0 = core.fake_dispatch_count()
    assert core.tmn_dispatch(s, H, 2, n_dests, local, 0) == TM_OK
    assert core.fake_dispatch_count() - c0 == 1 and core.fake_set_reruns(s) == 1   # sticky sizes: no rerun
    assert deliveries(core, s) == (0, exp_dl)
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)
    core.fake_dispatch_mult(1)


def test_device_failure_is_a_device_error(core):
    core.fake_dispatch_mult(1)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    for topics in ([b"ab", b"!x", b"cd"], [b"ab", b"~x"]):
        assert pack(core, s, topics) == TM_OK
        assert core.tmn_dispatch(s, H, len(topics), 2, 0, 0) == TM_EDEVICE
        b, e = C.c_uint64(), C.c_uint64()
        assert core.tmn_route_dest(s, 0, C.byref(b), C.byref(e)) == TM_EINVAL   # no result to slice
        assert deliveries(core, s) == (TM_EINVAL, [])                           # and none to deliver
    assert pack(core, s, [b"ab", b"+x"]) == TM_OK
    assert core.tmn_dispatch(s, H, 2, 2, 1, 0) == TM_OK
    exp, exp_dl = expected([b"ab", b"+x"], 2, 1)
    assert slices(core, s, 2) == exp and deliveries(core, s) == (0, exp_dl)
    assert core.tmn_match(s, H, 2, 0) == TM_OK
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler (gcc) to build the NIF dispatch check")
    exe = tmp_path / "nif_dispatch_check"
    b = subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}",
                        "-o", str(exe)] + [str(s) for s in SOURCES] +
                       [str(ROOT / "tests" / "native" / "nif_dispatch_check.c")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"
